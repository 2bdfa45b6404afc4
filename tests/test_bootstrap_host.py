"""CPU: the host-only parts of NJ bootstrap support — dst_bootstrap_columns against the restated SplitMix64 map,
dst_newick_support's labelled text, and the `--bootstrap` / `--seed` surface of the CLI (help lines and usage errors,
reported before any GPU work)."""
import os
import subprocess

import numpy as np
import pytest

import bootstrap_reference as B
import distance_amd as da
import nj_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "distance_amd", "cli", "distance")


# ---- the column map ------------------------------------------------------------------------------------------------
def test_restatements_agree():
    """the numpy map is the formula in Python integers"""
    for seed in (0, 1, 12345, (1 << 64) - 1):
        for r in (0, 3, 1 << 31):
            for length in (1, 7, 1000):
                want = [B.column(seed, r * length + c, length) for c in range(length)]
                assert [int(x) for x in B.columns(seed, r, length)] == want


def test_column_of_first_output():
    """SplitMix64 seeded with 0: its first output is 0xE220A8397B1DCDAF; with len = 2^32 - 1 the column is that output's
    high half scaled, computed by hand"""
    z = 0xE220A8397B1DCDAF
    assert B.column(0, 0, 1 << 32) == z >> 32
    assert B.column(0, 0, (1 << 32) - 1) == (z * ((1 << 32) - 1)) >> 64


@pytest.mark.parametrize("seed", [0, 1, (1 << 64) - 1])
@pytest.mark.parametrize("replicate", [0, 1, 1 << 31])
@pytest.mark.parametrize("length", [1, 7, 30_000, (1 << 20) + 3])
def test_bootstrap_columns(seed, replicate, length):
    got = da.bootstrap_columns(seed, replicate, length)
    assert got.dtype == np.uint32 and got.shape == (length,)
    assert np.array_equal(got, B.columns(seed, replicate, length))
    for c in (0, length // 2, length - 1):
        assert int(got[c]) == B.column(seed, replicate * length + c, length)
    assert int(got.max()) < length


def test_columns_differ_between_replicates_and_seeds():
    a, b, c = da.bootstrap_columns(1, 0, 5000), da.bootstrap_columns(1, 1, 5000), da.bootstrap_columns(2, 0, 5000)
    assert not np.array_equal(a, b) and not np.array_equal(a, c)
    # drawn with replacement: about 1 - 1/e of the columns appear
    assert 0.6 < len(np.unique(a)) / 5000 < 0.66


# ---- labelled Newick -----------------------------------------------------------------------------------------------
def tree(n, seed):
    d = np.random.default_rng(seed).random((n, n))
    return R.nj(d)


@pytest.mark.parametrize("n", [3, 4, 9, 120])
def test_newick_support_round_trip(n):
    parent, length = tree(n, n)
    ids = [f"r{k}" for k in range(n - 1)] + ["it's (x)"]
    sup = np.random.default_rng(n).integers(0, 10001, 2 * n - 2).astype(np.uint32)
    sup[:n] = 0xFFFFFFFF
    sup[2 * n - 3] = 0xFFFFFFFF
    text = da.newick(parent, length, ids, support=sup)
    plain = da.newick(parent, length, ids)
    assert da.newick(parent, length, ids, support=None) == plain
    assert B.strip_labels(text) == plain
    assert text.count(b")") == n - 1 and text.endswith(b";\n")
    names, p2, l2, lab = B.parse_labelled(text)
    assert sorted(names) == sorted(ids)
    # the same tree: leaf splits by name, and every internal node's label and length with its split
    order = [ids.index(x) for x in names]   # parsed leaf k is record order[k]

    def keyed(par, lens, labels, leaf_ids, nleaves):
        below = B._below(par, nleaves)
        full = (1 << n) - 1
        out = {}
        for x in range(nleaves, len(par)):
            if int(par[x]) == B.ROOT_PARENT:
                continue
            m = sum(1 << leaf_ids[k] for k in range(nleaves) if below[x] >> k & 1)
            out[m if not m & 1 else full ^ m] = (labels[x], round(float(lens[x]), 12))
        return out

    want = keyed(parent, length, list(sup), list(range(n)), n)
    got = keyed(p2, l2, lab, order, n)
    assert got == want
    for k in range(n):   # leaf lengths
        assert l2[k] == float(f"{length[order[k]]:.12f}")


def test_newick_support_errors():
    parent, length = tree(6, 1)
    sup = np.zeros(10, np.uint32)
    bad = parent.copy()
    bad[2] = bad[3]   # three children somewhere
    bad[4] = 10
    with pytest.raises(da.DistanceError):
        da.newick(bad, length, list("abcdef"), support=sup)
    with pytest.raises(ValueError):
        da.newick(parent, length, list("abcdef"), support=sup[:9])


# ---- CLI -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def cli():
    if not os.path.exists(CLI):
        subprocess.run(["make", "-C", os.path.dirname(CLI)], check=True)
    return CLI


def test_help_lines(cli):
    r = subprocess.run([cli, "-h"], capture_output=True)
    assert r.returncode == 0
    lines = r.stdout.decode().splitlines()
    for flag, meta in (("--bootstrap", "<B>"), ("--seed", "<S>")):
        mine = [x for x in lines if x.lstrip().startswith(flag + " ")]
        assert len(mine) == 1 and meta in mine[0], lines
        for other in ("--tree", "--matrix", "--clusters", "--nearest"):
            assert other not in mine[0]
    assert "10000" in [x for x in lines if "--bootstrap" in x][0]


@pytest.mark.parametrize("args", [
    ["--bootstrap", "10", "{a}"], ["--bootstrap=5", "--clusters", "3", "{a}"], ["--bootstrap", "5", "--matrix", "tsv", "{a}"],
    ["--tree", "nj", "--seed", "3", "{a}"], ["--seed", "3", "{a}"],
    ["--tree", "nj", "--bootstrap", "0", "{a}"], ["--tree", "nj", "--bootstrap", "10001", "{a}"],
    ["--tree", "nj", "--bootstrap", "-1", "{a}"], ["--tree", "nj", "--bootstrap", "abc", "{a}"],
    ["--tree", "nj", "--bootstrap", "", "{a}"], ["--tree", "nj", "--bootstrap", "1e2", "{a}"], ["--tree", "nj", "--bootstrap"],
    ["--tree", "nj", "--bootstrap", "5", "--seed", "-1", "{a}"],
    ["--tree", "nj", "--bootstrap", "5", "--seed", "18446744073709551616", "{a}"],
    ["--tree", "nj", "--bootstrap", "5", "--seed", "x", "{a}"], ["--tree", "nj", "--bootstrap", "5", "--seed"],
    ["--tree", "nj", "--bootstrap", "5", "{a}", "{b}"], ["--tree", "nj", "--bootstrap", "5", "-i", "{a}", "-s", "{b}"],
    ["--tree", "nj", "--bootstrap", "5", "--gpus", "2", "{a}"], ["--tree", "nj", "--bootstrap", "5", "--devices", "0,1", "{a}"],
    ["--tree", "nj", "--bootstrap", "5", "--nearest", "2", "{a}"],
    ["--tree", "upgma", "--bootstrap", "5", "{a}"],
])
def test_usage_errors(cli, tmp_path, args):
    for name in ("a", "b"):
        (tmp_path / f"{name}.fasta").write_bytes(b">x\nACGT\n>y\nACGA\n>z\nACCA\n")
    args = [x.replace("{a}", str(tmp_path / "a.fasta")).replace("{b}", str(tmp_path / "b.fasta")) for x in args]
    r = subprocess.run([cli] + args, capture_output=True, env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))
    assert r.returncode == 2, (args, r.stderr.decode())
    assert r.stdout == b""
    assert r.stderr.startswith(b"error: "), r.stderr
