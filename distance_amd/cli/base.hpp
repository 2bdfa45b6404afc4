// What every part of the CLI uses: the ways out, the context check, phase timing, the CPU count.
// (The headers of this directory other than fasta.hpp / format.hpp are the parts of main.cpp's one translation unit.)
#pragma once
#include <algorithm>
#include <cerrno>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>

#include <unistd.h>

#include "../../include/distance_hip.h"

namespace {

const char *kVersion = "0.3.1";  // Cargo.toml:3 of the reference this CLI mirrors

// ---------------------------------------------------------------- errors ----------------------
// main() of the reference returns Result<(), DistanceError>: Rust prints `Error: {:?}` and exits 1.
// Fatal errors can surface on a reader / worker thread while GPU threads are still running: flush
// what was written (the reference's BufWriter content is flushed on its way out too) and leave
// without running static destructors under those threads.
[[noreturn]] void leave(int code)
{
    std::fflush(nullptr);
    _exit(code);
}

[[noreturn]] void die_message(const std::string &m)
{
    std::fprintf(stderr, "Error: Message(\"%s\")\n", m.c_str());
    leave(1);
}

[[noreturn]] void die_io(const std::string &what, int err)
{
    std::fprintf(stderr, "Error: IOError(Os { code: %d, kind: %s, message: \"%s\" }) [%s]\n", err,
                 err == ENOENT ? "NotFound" : err == EACCES ? "PermissionDenied" : "Other", std::strerror(err),
                 what.c_str());
    leave(1);
}

[[noreturn]] void die_usage(const std::string &m)
{
    std::fprintf(stderr, "error: %s\n\nFor more information, try '--help'.\n", m.c_str());
    std::exit(2);  // clap's usage-error exit code
}

struct Ctx {
    dst_ctx *h = nullptr;
    void check(int rc, const char *what) const
    {
        if (rc != DST_OK) {
            std::fprintf(stderr, "Error: Gpu(\"%s: %s\")\n", what, dst_last_error(h));
            leave(1);
        }
    }
};

// DISTANCE_TIMING=1: phase wall times on stderr
struct PhaseTimer {
    bool on = std::getenv("DISTANCE_TIMING") != nullptr;
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), last = t0;
    void mark(const char *what)
    {
        if (!on)
            return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[timing] %-28s %8.1f ms (total %8.1f ms)\n", what,
                     std::chrono::duration<double, std::milli>(now - last).count(),
                     std::chrono::duration<double, std::milli>(now - t0).count());
        last = now;
    }
};

// num_cpus::get() (src/lib.rs:262): the CPUs this process may use — its affinity mask, capped by a cgroup CPU
// quota when the container has one (cgroup v2 cpu.max, v1 cpu.cfs_quota_us / cpu.cfs_period_us).
size_t available_cpus()
{
    size_t n = std::max<unsigned>(1, std::thread::hardware_concurrency());
    auto quota = [](const char *path_quota, const char *path_period) -> double {
        double q = -1, p = 100000;
        if (FILE *fh = std::fopen(path_quota, "r")) {
            char word[64] = {0};
            if (path_period == nullptr) {  // "max 100000" or "1600000 100000"
                double per = 0;
                if (std::fscanf(fh, "%63s %lf", word, &per) == 2 && std::strcmp(word, "max") != 0) {
                    q = std::atof(word);
                    p = per;
                }
            } else if (std::fscanf(fh, "%lf", &q) != 1) {
                q = -1;
            }
            std::fclose(fh);
        }
        if (path_period)
            if (FILE *fh = std::fopen(path_period, "r")) {
                if (std::fscanf(fh, "%lf", &p) != 1)
                    p = 100000;
                std::fclose(fh);
            }
        return (q > 0 && p > 0) ? q / p : -1.0;
    };
    double c = quota("/sys/fs/cgroup/cpu.max", nullptr);
    if (c < 0)
        c = quota("/sys/fs/cgroup/cpu/cpu.cfs_quota_us", "/sys/fs/cgroup/cpu/cpu.cfs_period_us");
    if (c > 0)
        n = std::min<size_t>(n, std::max<size_t>(1, (size_t)(c + 0.999)));
    return n;
}

}  // namespace
