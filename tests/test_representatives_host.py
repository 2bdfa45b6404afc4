"""CPU: greedy representatives without a GPU — the sequential reference (representatives_reference.py) on hand-worked
graphs and its stated consequences on random graphs; dst_representatives declared, exported and typed; the ABI version;
the `--representatives T` help line and every usage error, which parse_args reports (exit 2, `error: ...`, nothing on
stdout) before any GPU work."""
import os
import subprocess

import numpy as np
import pytest

import distance_amd as da
import representatives_reference as rr
from distance_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


@pytest.fixture(scope="module", autouse=True)
def built():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)


def rep_of(n, edges, t=1):
    vals = rr.condensed(n, edges)
    return rr.reference("n_high", vals, n, t)


# ---- the reference on hand-worked graphs ------------------------------------------------------------------------------------
def test_path():
    # 0 - 1 - 2 - 3 - 4 - 5 - 6: every second record is kept, each odd one stands behind its left neighbour
    n = 7
    rep, values, _ = rep_of(n, [(k, k + 1) for k in range(n - 1)])
    assert list(rep) == [0, 0, 2, 2, 4, 4, 6]
    assert list(values) == [0, 1, 0, 1, 0, 1, 0]


def test_star():
    # centre 3: at T = 1 record 0 is kept first and takes the centre; every other leaf is only linked to the centre, a member
    n = 6
    rep, values, _ = rep_of(n, [(3, k) for k in range(n) if k != 3])
    assert list(rep) == [0, 1, 2, 0, 4, 5]
    assert list(values) == [0, 0, 0, 1, 0, 0]
    # centre 0: one representative
    rep, _, _ = rep_of(n, [(0, k) for k in range(1, n)])
    assert list(rep) == [0] * n


def test_two_hubs():
    # a = 0 and b = 1 are not linked; every later record is linked to both: the smaller hub wins, with its own value
    n = 8
    vals = rr.condensed(n, [], rest=9)
    for k in range(2, n):
        vals[rr.row_start(n, 0) + k - 1] = 2 if k % 2 else 1       # (0, k)
        vals[rr.row_start(n, 1) + k - 2] = 1 if k % 2 else 2       # (1, k)
    rep, values, _ = rr.reference("n_high", vals, n, 2)
    assert list(rep) == [0, 1] + [0] * (n - 2)
    assert list(values) == [0, 0] + [2 if k % 2 else 1 for k in range(2, n)]


def test_ambiguity_is_not_transitive():
    # A, R, G at one site: d(0, 1) = d(1, 2) = 0 and d(0, 2) = 1.  One single-linkage cluster, two representatives.
    vals = np.array([0, 1, 0], np.int64)   # (0, 1), (0, 2), (1, 2)
    rep, values, _ = rr.reference("n_high", vals, 3, 0)
    assert list(rep) == [0, 0, 2] and list(values) == [0, 0, 0]


def test_member_of_a_member_is_not_covered():
    # 0 - 1 - 2: record 1 is a member, so its link to 2 covers nothing and 2 is kept
    rep, _, _ = rep_of(3, [(0, 1), (1, 2)])
    assert list(rep) == [0, 0, 2]


def test_link_rule():
    v = np.array([0.0, -0.0, 1.5, np.nan, np.inf])
    assert list(rr.linked("raw", v, 0.0)) == [True, True, False, False, False]
    assert list(rr.linked("raw", v, -0.0)) == [True, True, False, False, False]
    assert list(rr.linked("raw", v, np.inf)) == [True, True, True, False, True]
    iv = np.array([0, 3, 4], np.int64)
    assert list(rr.linked("n", iv, 3.75)) == [True, True, False]
    assert not rr.linked("n", iv, -1e300).any() and rr.linked("n", iv, 1e300).all()
    assert not rr.linked("n_high", iv, -0.5).any()


def test_tallies_follow_the_values():
    n = 4
    vals = rr.condensed(n, [(0, 2), (1, 3)])
    tallies = np.arange(6 * 2, dtype=np.uint32).reshape(6, 2) + 1
    rep, values, tal = rr.reference("n_high", vals, n, 1, tallies)
    assert list(rep) == [0, 1, 0, 1]
    assert tal[0].tolist() == [0, 0] and tal[1].tolist() == [0, 0]
    assert tal[2].tolist() == tallies[1].tolist()      # pair (0, 2) is entry 1
    assert tal[3].tolist() == tallies[4].tolist()      # pair (1, 3) is entry 4


def components(n, link):
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x

    i, j = np.triu_indices(n, 1)
    for a, b in zip(i[link], j[link]):
        ra, rb = find(int(a)), find(int(b))
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(x) for x in range(n)], np.int64)


# ---- the six consequences on random graphs ---------------------------------------------------------------------------------
@pytest.mark.parametrize("n,density,seed", [(1, 0.5, 1), (2, 0.5, 2), (40, 0.0, 3), (40, 0.03, 4), (60, 0.1, 5), (60, 0.5, 6),
                                            (30, 1.0, 7), (90, 0.02, 8)])
def test_consequences_on_random_graphs(n, density, seed):
    rng = np.random.default_rng(seed)
    link = rng.random(n * (n - 1) // 2) < density
    rep = rr.greedy(n, link)
    rr.check_consequences(n, link, rep, components(n, link))
    nb = np.zeros((n, n), bool)
    i, j = np.triu_indices(n, 1)
    nb[i, j] = link
    nb |= nb.T
    assert np.array_equal(rr.greedy_from_neighbours(n, lambda x: np.nonzero(nb[x])[0]), rep)


# ---- the library's surface ----------------------------------------------------------------------------------------------------
def test_declared_and_exported():
    assert "dst_representatives" in da.declared_symbols()
    lib = da.load()
    assert hasattr(lib, "dst_representatives")
    assert "dst_representatives" in _lib._SIGS
    assert len(_lib._SIGS["dst_representatives"][1]) == 9
    assert hasattr(da.Engine, "representatives")


def test_abi_version_stays_3():
    assert da.load().dst_abi_version() == 3


def test_header_states_the_consequences():
    text = open(_lib.HEADER_PATH).read()
    at = text.index("greedy representatives")
    block = text[at:text.index("int dst_representatives(", at)]
    for phrase in ("no two representatives are linked", "record 0 is always a representative",
                   "smallest record of every dst_clusters(T) cluster is a representative"):
        assert phrase in " ".join(block.replace("*", " ").split()), phrase


# ---- the command line ------------------------------------------------------------------------------------------------------------
def test_help_lists_representatives():
    r = subprocess.run([CLI, "-h"], capture_output=True)
    assert r.returncode == 0
    line = [x for x in r.stdout.decode().splitlines() if "--representatives" in x]
    assert len(line) == 1 and "<T>" in line[0]


OTHER_MODES = [["--nearest", "2"], ["--closest", "2"], ["--closest-for", "loaded"], ["--within", "1"], ["--clusters", "1"],
               ["--max-distance", "1"], ["--summary", "1"], ["--groups", "{g}"], ["--groups-within", "1"], ["--per-record"],
               ["--histogram", "1"], ["--bins", "8"], ["--matrix", "tsv"], ["--tree", "nj"], ["--bootstrap", "5"], ["--seed", "3"],
               ["--mst"], ["--sites"], ["--dendrogram", "average"]]


@pytest.mark.parametrize("args", [
    ["--representatives", "x"], ["--representatives", "nan"], ["--representatives", "-1"], ["--representatives", "-inf"],
    ["--representatives", ""], ["--representatives", "3x"], ["--representatives", " 3"], ["--representatives=1,5"],
    ["--representatives"],
    ["--representatives", "3", "{b}"], ["--representatives", "3", "-i", "{a}", "{b}"],
    ["--representatives", "3", "-s", "{b}"], ["-s", "{b}", "--representatives", "3"],
    ["--representatives", "3", "--gpus", "2"], ["--representatives", "3", "--devices", "0,1"],
    ["--representatives", "3", "--representatives", "3"], ["--representatives=3", "--representatives=4"],
] + [["--representatives", "3"] + m for m in OTHER_MODES] + [m + ["--representatives", "3"] for m in OTHER_MODES])
def test_usage_errors(tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    (tmp_path / "g.tsv").write_bytes(b"x\tone\ny\ttwo\n")
    sub = {"{a}": str(tmp_path / "a.fasta"), "{b}": str(tmp_path / "b.fasta"), "{g}": str(tmp_path / "g.tsv")}
    args = [sub.get(x, x) for x in args]
    if "-i" not in args:
        args.append(str(tmp_path / "a.fasta"))
    r = subprocess.run([CLI] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr


@pytest.mark.parametrize("mode", OTHER_MODES)
def test_the_new_row_speaks_first(tmp_path, mode):
    """Every combination is refused by --representatives' own row, whichever flag comes first on the line."""
    (tmp_path / "a.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n")
    (tmp_path / "g.tsv").write_bytes(b"x\tone\ny\ttwo\n")
    mode = [str(tmp_path / "g.tsv") if x == "{g}" else x for x in mode]
    for args in (["--representatives", "3"] + mode, mode + ["--representatives", "3"]):
        r = subprocess.run([CLI] + args + [str(tmp_path / "a.fasta")], capture_output=True,
                           env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
        assert r.returncode == 2
        first = r.stderr.decode().splitlines()[0]
        assert first.startswith("error: the argument '--representatives <T>' cannot be used with '" + mode[0]), first
