"""pb_slot_select (pb_select.hip): dst <- src for the filters whose mask entry equals `when`, every other filter's column of dst
untouched -- bit for bit against numpy's np.where on what pb_get_slot / pb_get_head read before and after.  15 and 21 states; a single
filter, a ragged last tile (100) and 65 536 filters; the mask on the host and on the device; checkpoint slots and the head on either
side; the error paths."""
import ctypes as C

import numpy as np
import pytest

from pronto_amd import _lib
from pronto_amd.synth import Workload

pytestmark = pytest.mark.gpu
HEAD = _lib.PB_SLOT_HEAD


def _read(est, slot):
    v, q, P, ll = est.get_head() if slot == HEAD else est.get_slot(slot)
    return v, q, P, ll


def _setup(n, B):
    """a context whose head and checkpoint slots 0..2 all hold different posteriors"""
    from pronto_amd.batch import BatchEstimator
    w = Workload(B, n_states=n)
    vec, quat, P0 = w.initial_state()
    q4 = w.process_noise()
    est = BatchEstimator(B, n_states=n)
    est.reset(vec, quat, P0)
    est.history_reserve(3)
    for k in range(4):
        est.predict(w.imu_block(k), q4)
        lo, mask = w.legodo_block(k)
        est.update_indexed([3, 4, 5], np.ascontiguousarray(lo[0:3]), np.ascontiguousarray(lo[3:6]), mask=mask)
        if k < 3:
            est.state_save(k)
    return est


def _check(est, dst, src, mask, when, device):
    import torch
    before = _read(est, dst)
    source = _read(est, src)
    if device:
        m = torch.from_numpy(mask).to("cuda:0")
        torch.cuda.synchronize()
    else:
        m = mask
    est.slot_select(dst, src, m, when)
    est.sync()
    after = _read(est, dst)
    sel = (mask != 0) == bool(when)
    for a, b, s in zip(after, before, source):
        want = np.where(sel, s, b)     # (the filter index is the last axis of every block)
        assert a.tobytes() == want.tobytes()
    return int(sel.sum())


@pytest.mark.parametrize("n", [15, 21])
@pytest.mark.parametrize("B", [1, 100, 65536])
def test_slot_select_is_a_bit_exact_masked_copy(n, B):
    est = _setup(n, B)
    rng = np.random.default_rng(B + n)
    cases = [(1, 0, 1, False), (2, HEAD, 0, True), (HEAD, 1, 1, True), (0, 2, 0, False)]
    if B < 65536:
        cases += [(1, HEAD, 1, False), (HEAD, 2, 0, False), (0, 1, 0, True), (2, 0, 1, True)]
    seen = set()
    for dst, src, when, device in cases:
        mask = (rng.random(B) < 0.5).astype(np.uint8) * rng.integers(1, 256, B).astype(np.uint8)   # (any non-zero entry counts as 1)
        if B == 1:
            mask[0] = len(seen) % 2
        nsel = _check(est, dst, src, mask, when, device)
        seen.add(nsel > 0)
    assert B == 1 or seen == {True}
    # nothing and everything selected
    _check(est, 0, 1, np.zeros(B, np.uint8), 1, False)
    _check(est, 0, 1, np.ones(B, np.uint8), 1, True)
    # dst == src (also the head's own slot): nothing moves
    _check(est, 1, 1, np.ones(B, np.uint8), 1, False)
    est.close()


def test_slot_select_error_paths():
    est = _setup(15, 70)
    L, h = est._L, est._h
    mask = np.ones(70, np.uint8)
    p = C.c_void_p(mask.ctypes.data)
    assert L.pb_slot_select(h, 3, 0, p, 1, _lib.PB_HOST) == _lib.PB_ERR_STATE        # slot out of range
    assert L.pb_slot_select(h, 0, -2, p, 1, _lib.PB_HOST) == _lib.PB_ERR_STATE
    assert L.pb_slot_select(h, 0, 1, None, 1, _lib.PB_HOST) == _lib.PB_ERR_ARG       # NULL mask
    assert b"NULL mask" in L.pb_last_error(h)
    assert L.pb_slot_select(h, 0, 1, p, 2, _lib.PB_HOST) == _lib.PB_ERR_ARG          # when = 2
    assert L.pb_slot_select(h, 0, 1, p, 1, _lib.PB_HOST_BROADCAST) == _lib.PB_ERR_ARG
    assert L.pb_slot_select(None, 0, 1, p, 1, _lib.PB_HOST) == _lib.PB_ERR_ARG
    assert L.pb_smooth_step_masked(h, 0, 1, 2, 0, 1e-3, p, _lib.PB_HOST) == _lib.PB_ERR_ARG   # slot_out = slot_next_pred
    est.close()
