"""pronto::error_metrics_t on the wire (pronto_amd/csrc/pronto_wire.hpp) against a struct.pack image and the independent
fingerprint of tests/lcm_ref.py.  CPU only."""
import math
import os
import struct
import subprocess

import pytest

import lcm_ref as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# pronto_error_metrics_t.lcm, member by member
ERROR_METRICS_T = [("utime", "int64_t", []), ("pos_error", "double", [(0, "3")]), ("pos_error_norm", "double", []),
                   ("rpy_error", "double", [(0, "3")]), ("distance_travelled", "double", []), ("percent_ddt", "double", []),
                   ("time_elapsed", "double", [])]
UTIME = 123456789012
FIELDS = [(i + 1) * 0.125 - 1.0 for i in range(10)]
FIELDS[8] = math.inf


@pytest.fixture(scope="module")
def tool():
    exe = os.path.join(ROOT, "tests", "build", "score_wire_tool")
    src = os.path.join(ROOT, "tests", "cpp", "score_wire_tool.cpp")
    hdr = os.path.join(ROOT, "pronto_amd", "csrc", "pronto_wire.hpp")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or os.path.getmtime(exe) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-o", exe, src])
    return exe


def image():
    return struct.pack(">Qq10d", L.fingerprint(ERROR_METRICS_T), UTIME, *FIELDS)


def decode(tool, tmp_path, blob):
    path = str(tmp_path / "in.bin")
    open(path, "wb").write(blob)
    return subprocess.check_output([tool, "decode", path], text=True).split()


def test_fingerprint(tool):
    assert int(subprocess.check_output([tool, "hash"], text=True), 16) == L.fingerprint(ERROR_METRICS_T)
    assert L.fingerprint(ERROR_METRICS_T) not in (L.fingerprint(L.FILTER_STATE_T), L.fingerprint(L.UPDATE_T))


def test_encode_equals_struct_pack_image(tool, tmp_path):
    path = str(tmp_path / "out.bin")
    subprocess.check_call([tool, "encode", path])
    assert open(path, "rb").read() == image()
    assert len(image()) == 8 + 8 + 10 * 8


def test_decode_round_trip(tool, tmp_path):
    out = decode(tool, tmp_path, image())
    assert int(out[0]) == len(image()) and int(out[1]) == UTIME
    assert [float(x) for x in out[2:]] == FIELDS


def test_truncated_and_wrong_fingerprint(tool, tmp_path):
    WIRE_ERR_SHORT, WIRE_ERR_FINGERPRINT = -1, -2
    assert decode(tool, tmp_path, image()[:-1]) == [str(WIRE_ERR_SHORT)]
    assert decode(tool, tmp_path, image()[:5]) == [str(WIRE_ERR_SHORT)]
    assert decode(tool, tmp_path, struct.pack(">Q", L.fingerprint(L.UPDATE_T)) + image()[8:]) == [str(WIRE_ERR_FINGERPRINT)]
