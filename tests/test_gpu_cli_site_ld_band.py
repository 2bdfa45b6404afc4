"""GPU (-m gpu): `distance --ld R2 --ld-max-gap G` against the plain `--ld R2` output filtered by site2 - site1 <= G, byte for
byte, and `--ld R2 --ld-decay W --ld-bins B` against site_ld_band_reference's text: one and three groups, a minimum count,
stdin, -o, and slabs of any size.  The alignment is test_gpu_cli_site_ld's."""
import pytest

from site_ld_band_reference import decay_text
from site_ld_reference import ld_text, tallies
from test_gpu_cli_site_ld import al, built, fmt, run  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu


def within(text, gap):
    """the header and the lines with site2 - site1 <= gap"""
    lines = text.splitlines(keepends=True)
    return lines[0] + "".join(x for x in lines[1:] if int(x.split("\t")[1]) - int(x.split("\t")[0]) <= gap)


@pytest.mark.parametrize("gap", [0, 1, 9, 60, 299, 100000])
def test_max_gap_one_group(al, gap, tmp_path):
    plain = run(["--ld", "0.2", "--ld-min-count", "2", al["fasta"]])
    assert plain == ld_text(al["codes"], 0.2, 2, fmt=fmt)
    want = within(plain, gap)
    assert run(["--ld", "0.2", "--ld-min-count", "2", "--ld-max-gap", str(gap), al["fasta"]]) == want
    if gap == 0:
        assert want.count("\n") == 1
    if gap == 60:
        assert 1 < want.count("\n") < plain.count("\n")
        out = tmp_path / "out.tsv"
        assert run(["--ld", "0.2", "--ld-max-gap=60", "--ld-min-count", "2", "-o", str(out), al["fasta"]]) == "" and out.read_text() == want
        with open(al["fasta"], "rb") as fh:
            assert run(["--ld-max-gap", "60", "--ld", "0.2", "--ld-min-count", "2"], stdin=fh) == want
        for slab in ("1", "7", "100"):
            assert run(["--ld", "0.2", "--ld-min-count", "2", "--ld-max-gap", "60", "--slab-pairs", slab, al["fasta"]]) == want
    if gap >= 299:
        assert want == plain


@pytest.mark.parametrize("gap", [5, 40])
def test_max_gap_three_groups(al, gap):
    base = ["--ld", "0", "--ld-groups", al["labels_file"], "--ld-min-count", "1"]
    plain = run(base + [al["fasta"]])
    assert plain == ld_text(al["codes"], 0.0, 1, al["labels"], al["names"], fmt=fmt)
    want = within(plain, gap)
    assert "\tz\t" in want and "\tx\t" in want and want != plain
    assert run(base + ["--ld-max-gap", str(gap), al["fasta"]]) == want
    assert run(base + ["--ld-max-gap", str(gap), "--slab-pairs", "50", al["fasta"]]) == want


@pytest.mark.parametrize("width, bins", [(1, 4096), (10, 7), (300, 1), (7, None)])
def test_decay(al, width, bins, tmp_path):
    codes = al["codes"]
    flags = ["--ld-decay", str(width)] + ([] if bins is None else ["--ld-bins", str(bins)])
    n_bins = 256 if bins is None else bins

    def tallies_of(groups):
        return lambda sites, allele, g: tallies(codes, sites, allele, groups, g)

    want = decay_text(codes, tallies_of(None), 0.2, width, n_bins, 2, fmt=fmt)
    assert want.count("\n") == 1 + n_bins and ("\tNaN\n" in want) == (width * n_bins > 400)   # (bins past the alignment's 300 sites)
    assert run(["--ld", "0.2", "--ld-min-count", "2"] + flags + [al["fasta"]]) == want
    assert run(["--ld", "0.2", "--ld-min-count", "2", "--slab-pairs", "9"] + flags + [al["fasta"]]) == want
    # three groups; group y lists fewer than two sites and prints nothing
    want = decay_text(codes, tallies_of(al["labels"]), 0.5, width, n_bins, 1, al["labels"], al["names"], fmt=fmt)
    assert want.count("\n") == 1 + 2 * n_bins and "\ny\t" not in want
    assert run(["--ld", "0.5", "--ld-groups", al["labels_file"]] + flags + [al["fasta"]]) == want
    if bins == 7:
        out = tmp_path / "out.tsv"
        assert run(["--ld", "0.5", "--ld-groups", al["labels_file"], "-o", str(out)] + flags + [al["fasta"]]) == "" and out.read_text() == want
        with open(al["fasta"], "rb") as fh:
            assert run(["--ld", "0.5", "--ld-groups", al["labels_file"], "--slab-pairs", "3"] + flags, stdin=fh) == want
