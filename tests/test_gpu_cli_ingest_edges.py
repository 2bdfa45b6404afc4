"""GPU (-m gpu): the `distance` CLI in stream mode at the widths where its own encoder for the 4-bit wire format (pack()
in distance_amd/cli/stream.hpp) takes its odd-width branch, and on both sides of a chunk's edge — on both wire formats, the
TSV byte for byte the text built from the oracle as test_gpu_cli.py builds it."""
import os
import subprocess

import pytest

import ingest_edge_cases as ic
import oracle
from test_gpu_cli import CLI, built, to_text, write_fasta   # noqa: F401  (built: the module's autouse fixture)

pytestmark = pytest.mark.gpu
WIDTHS = (1, 2, 3, 5, 7, 129, 131)


@pytest.mark.parametrize("measure", ("n", "tn93"))
@pytest.mark.parametrize("L", WIDTHS)
def test_stream_mode_text_at_odd_widths_on_both_wires(tmp_path, L, measure):
    a, b = ic.loaded_set(L), ic.case_rows(L, 3)
    ida, idb = [f"a{i}" for i in range(len(a))], [f"b{i}" for i in range(len(b))]
    fa, fb = tmp_path / "a.fa", tmp_path / "b.fa"
    write_fasta(fa, ida, to_text(a))
    write_fasta(fb, idb, to_text(b))
    d = oracle.all_pairs_rect(measure, a, b, counts_a=oracle.count_bases_matrix(a), counts_b=oracle.count_bases_matrix(b))
    ij = [(i, j) for j in range(len(b)) for i in range(len(a))]              # streamed record outer
    want = oracle.tsv(ida, idb, ij, [int(d[i, j]) if measure in oracle.INT_MEASURES else d[i, j] for i, j in ij])
    for wire in ("codes", None):                                              # None: the default, the codes' high nibbles
        env = dict(os.environ)
        env.pop("DISTANCE_WIRE", None)
        if wire:
            env["DISTANCE_WIRE"] = wire
        r = subprocess.run([CLI, "-m", measure, "-i", str(fa), "-s", str(fb)], capture_output=True, env=env)
        assert r.returncode == 0, r.stderr.decode()
        assert r.stdout.decode() == want, (L, measure, wire or "nibbles")
