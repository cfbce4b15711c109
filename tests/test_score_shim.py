"""DriftPerDistance through the C++ mirror (tests/cpp/test_score.cpp): a miniature se-fusion with ins + legodo and
fuse_ins_legodo = true on written event logs with a ground-truth pose channel.

The executable replays every log twice -- once with the handler as the subscribePose callback, once downloading getHeadState at
every ground-truth message, making that head the head of a second context (pb_set_head) and scoring it there -- and the two score
states must be identical, bit for bit, rows and counts (a handler that did not apply the held INS step would score another head).
The g++ build of the per-lane functions runs on the same downloaded heads as an extra check, with the bounds every comparison of
the device code with its host build uses (counts, utimes and anchors identical, lengths and angles 1e-12, percent_ddt 1e-9).
"segments": 8 logs of different lengths through SegmentBatcher; a segment
that has ended stops accumulating."""
import subprocess

import pytest

from test_cpp_shim import build_exe


def test_shim_compiles_and_links(oracle):
    exe = build_exe(oracle, "test_score")
    out = subprocess.run(["ldd", exe], capture_output=True, text=True).stdout
    assert "libpronto_batch.so" in out and "not found" not in out.split("libpronto_batch.so")[1].split("\n")[0]


@pytest.mark.gpu
@pytest.mark.parametrize("n,mode", [(15, "player"), (21, "player"), (15, "segments"), (21, "segments")])
def test_handler_against_head_download(oracle, tmp_path, n, mode):
    exe = build_exe(oracle, "test_score")
    r = subprocess.run([exe, str(tmp_path), "n%d" % n] + (["segments"] if mode == "segments" else []), capture_output=True, text=True, timeout=300)
    print(r.stdout[-3000:], r.stderr[-2000:])
    assert r.returncode == 0 and "PASS" in r.stdout, r.stdout[-3000:] + r.stderr[-2000:]
