"""The optical-flow sigma-point update on the device (pb_update_optical_flow, pronto_amd/csrc/rbis_flow_kernels.hpp) -- run with
`-m gpu` on an MI355X.  B = 130: two full waves and a two-lane tail; 15 and 21 states.

  exact      the posterior and zhat_out against 60-digit arithmetic under flow_ref.judge's bound (16 x the unreduced numpy witness's
             error + 1e-13 per piece and bin of cond(Pzz); the filters without an exact result within 17 x of the witness), flags 0
             and 1, per-filter diagonal R; a host diagonal and a full R with off-diagonals likewise.  In the batch, in a wave's body
             and in the tail: a filter whose sigma points all stay below the chi fold tolerance, one with P = 0 (status 2), one whose
             pivot 7 is negative (status 9); the skipped ones keep every bit.  Quaternion and log-likelihood keep the prior's bits.
  spaces     one message for every filter as PB_HOST blocks, PB_DEVICE tensors and PB_HOST_BROADCAST values, R as a host diagonal, a
             per-filter diagonal and a full matrix: equal bits
  mask/slots masked-off filters keep every bit (status 1); the output slot is honoured; two runs agree bit for bit
  refusals   a pending predicted slot, a call before pb_flow_set_camera, unknown flags, a mask with a broadcast message
  tail       a second batch with the negative pivot 7 at 70 and in the tail (129): statuses, kept bits, every other filter as before
  predict    one pb_predict behind the update equals the oracle's predict from the device's own read-back posterior at 1e-9: the chi
             the update leaves in the vector is folded by the next addState"""
import ctypes as C

import numpy as np
import pytest

import flow_ref as fr
from test_gpu_parity import pa  # noqa: F401  (the module fixture that builds and imports the package)

pytestmark = pytest.mark.gpu

B = fr.B_GPU
NS = [15, 21]
PB_HOST, PB_ERR_ARG, PB_ERR_STATE = 0, 1, 4


def _estimator(pa, oracle, n, h, slots=0, camera=True):
    est = pa.BatchEstimator(B, n_states=n)
    g, tol = oracle.constants()
    assert tol == fr.TOL
    est.set_constants(g, tol)
    if slots:
        est.history_reserve(slots)
    if camera:
        est.flow_set_camera(*fr.camera())
    _set_head(est, h)
    return est


def _set_head(est, h):
    """the head with its log-likelihood (pb_reset zeroes it)"""
    est.reset(h["vec"], h["quat"], np.ascontiguousarray(h["P"]))
    v, q, P, ll = (np.ascontiguousarray(h[k]) for k in ("vec", "quat", "P", "ll"))
    rc = est._L.pb_set_head(est._h, v.ctypes.data, q.ctypes.data, P.ctypes.data, ll.ctypes.data, PB_HOST)
    assert rc == 0, est._L.pb_last_error(est._h)


def _got(est, zhat, status):
    v, q, P, ll = est.get_head()
    return dict(vec=v, quat=q, P=P, ll=ll, zhat=zhat.cpu().numpy(), status=status.cpu().numpy())


def _same_bits(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def _run_case(pa, oracle, n, flags, kind):
    c = fr.reference(n, flags, kind)
    fr.assert_input_conditions(c)
    est = _estimator(pa, oracle, n, c.h)
    R = list(c.R) if kind == "host" else c.R
    got = _got(est, *est.update_optical_flow(c.h["flow"], R, flags=flags, want_zhat=True, want_status=True))
    est.close()
    assert np.array_equal(got["quat"], c.h["quat"]) and np.array_equal(got["ll"], c.h["ll"])        # the prior's bits
    assert np.all(np.isnan(got["zhat"][:, got["status"] != 0])) and np.all(np.isfinite(got["zhat"][:, got["status"] == 0]))
    st = got["status"]
    assert set(st[list(fr.SPECIAL["zero"])]) == {2} and set(st[list(fr.SPECIAL["col7"])]) == {9} and set(st[list(fr.SPECIAL["fold"])]) == {0}
    fr.judge("gpu n=%d flags=%d R=%s" % (n, flags, kind), c, got)


@pytest.mark.parametrize("flags", [0, 1])
@pytest.mark.parametrize("n", NS)
def test_against_exact_arithmetic(pa, oracle, n, flags):
    _run_case(pa, oracle, n, flags, "diag")


@pytest.mark.parametrize("n,kind", [(15, "host"), (21, "full")])
def test_r_encodings_against_exact_arithmetic(pa, oracle, n, kind):
    _run_case(pa, oracle, n, 0, kind)


@pytest.mark.parametrize("n", NS)
def test_second_batch_with_the_negative_pivot_in_the_tail(pa, oracle, n):
    """B = 130 has a two-lane tail, which the first batch fills with `fold` and `zero`: here pivot 7 is negative at 70 and at 129"""
    got = []
    for h in (fr.add_specials(fr.heads(n)), fr.add_specials(fr.heads(n), fr.SPECIAL_TAIL7)):
        est = _estimator(pa, oracle, n, h)
        got.append(_got(est, *est.update_optical_flow(h["flow"], h["R"], want_zhat=True, want_status=True)))
        est.close()
    fr.check_second_batch(h, got[0], got[1])


@pytest.mark.parametrize("n", NS)
def test_input_spaces_and_r_encodings_give_equal_bits(pa, oracle, n):
    import torch
    h = fr.add_specials(fr.heads(n))
    msg, Rd = h["flow"][:, 0].copy(), h["R"][:, 0].copy()
    tile = lambda a: np.ascontiguousarray(np.tile(a[:, None], (1, B)))
    sums = []
    for space in ("host", "device", "broadcast"):
        for enc in ("list", "diag", "full"):
            R = list(Rd) if enc == "list" else (Rd if enc == "diag" else np.diag(Rd).T.ravel().copy())
            if space == "broadcast":
                flow = msg
            else:
                flow, R = tile(msg), (R if enc == "list" else tile(R))
                if space == "device":
                    flow, R = torch.from_numpy(flow).cuda(), (R if enc == "list" else torch.from_numpy(R).cuda())
            est = _estimator(pa, oracle, n, h)
            zhat, status = est.update_optical_flow(flow, R, want_zhat=True, want_status=True)
            sums.append((tuple(est.state_checksum()), zhat.cpu().numpy().tobytes(), status.cpu().numpy().tobytes()))
            est.close()
    assert all(s == sums[0] for s in sums)


@pytest.mark.parametrize("n", NS)
def test_mask_output_slot_and_repeatability(pa, oracle, n):
    h = fr.add_specials(fr.heads(n))
    mask = (np.arange(B) % 3 != 1).astype(np.uint8)          # masked-off filters in both waves and in the tail (127)
    mask[129] = 0
    est = _estimator(pa, oracle, n, h, slots=3)
    prior = est.get_head()
    _, st_plain = est.update_optical_flow(h["flow"], h["R"], want_status=True)
    plain = est.get_head()
    _set_head(est, h)
    zhat, status = est.update_optical_flow(h["flow"], h["R"], mask=mask, want_zhat=True, want_status=True)
    masked = est.get_head()
    status, st_plain = status.cpu().numpy(), st_plain.cpu().numpy()
    assert np.all(status[mask == 0] == 1) and np.array_equal(status[mask == 1], st_plain[mask == 1]) and np.all(np.isnan(zhat.cpu().numpy()[:, mask == 0]))
    assert all(np.array_equal(a[..., mask == 0], p[..., mask == 0]) for a, p in zip(masked, prior)), "a masked filter moved"
    assert all(np.array_equal(a[..., mask == 1], p[..., mask == 1]) for a, p in zip(masked, plain))
    assert not np.array_equal(plain[0][:, mask == 1], prior[0][:, mask == 1])
    # two runs agree bit for bit
    _set_head(est, h)
    est.update_optical_flow(h["flow"], h["R"], mask=mask)
    assert _same_bits(est.get_head(), masked)
    # the posterior through an output slot: the in-place result, the masked and the skipped filters' rows copied over, the head follows
    _set_head(est, h)
    est.set_output_slot(1)
    est.update_optical_flow(h["flow"], h["R"], mask=mask)
    assert est._L.pb_head_slot(est._h) == 1
    assert _same_bits(est.get_head(), masked) and _same_bits(est.get_slot(1), masked)
    # a head that lives in a slot: the next update goes back to the context's own array and leaves the slot as it was
    est.update_optical_flow(h["flow"], h["R"], mask=mask)
    assert est._L.pb_head_slot(est._h) == -1 and _same_bits(est.get_slot(1), masked)
    est.close()


def test_refusals(pa, oracle):
    h = fr.heads(15)
    est = _estimator(pa, oracle, 15, h, slots=2, camera=False)
    before = tuple(est.state_checksum())
    with pytest.raises(pa.PbError) as e:
        est.update_optical_flow(h["flow"], h["R"])
    assert e.value.code == PB_ERR_STATE and "pb_flow_set_camera" in str(e.value)
    est.flow_set_camera(*fr.camera())
    est.set_pred_slot(1)
    with pytest.raises(pa.PbError) as e:
        est.update_optical_flow(h["flow"], h["R"])
    assert e.value.code == PB_ERR_STATE
    with pytest.raises(pa.PbError) as e:
        est.update_optical_flow(h["flow"], h["R"], flags=2)
    assert e.value.code == PB_ERR_ARG
    with pytest.raises((pa.PbError, ValueError)):
        est.update_optical_flow(h["flow"][:, 0].copy(), list(h["R"][:, 0]), mask=np.ones(B, dtype=np.uint8))
    ones = np.ones(B, dtype=np.uint8)
    rc = est._L.pb_update_optical_flow(est._h, h["flow"][:, 0].copy().ctypes.data, h["R"][:, 0].copy().ctypes.data, 0, ones.ctypes.data, 2, 0, None, None)
    assert rc == PB_ERR_ARG
    with pytest.raises(ValueError):
        est.update_optical_flow(h["flow"][:6], h["R"])
    with pytest.raises(ValueError):
        est.flow_set_camera([0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1])
    assert tuple(est.state_checksum()) == before
    est.update_optical_flow(h["flow"], h["R"])                  # the refused slot is forgotten
    assert tuple(est.state_checksum()) != before
    est.close()


@pytest.mark.parametrize("n", NS)
def test_predict_after_the_update_folds_the_chi_it_left(pa, oracle, n):
    from pronto_amd.synth import Workload
    h = fr.heads(n)
    est = _estimator(pa, oracle, n, h)
    est.update_optical_flow(h["flow"], h["R"])
    v, q, P, ll = est.get_head()
    assert np.max(np.linalg.norm(v[6:9], axis=0)) > 10 * fr.TOL     # the update left a chi that the fold has to take
    w = Workload(B, n_states=n)
    imu = np.ascontiguousarray(w.streams(0, 1)[0][0])
    q4 = w.process_noise()
    est.predict(imu, q4)
    gv, gq, gP, gll = est.get_head()
    est.close()
    v21, P21 = np.zeros((21, B)), np.zeros((21, 21, B))
    v21[:n], P21[:n, :n] = v, P
    ob = oracle.OracleBatch(v21, q, P21, ll)
    ob.predict(imu, q4)
    rel = lambda a, b: float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))
    big = np.linalg.norm(v[6:9], axis=0) > 10 * fr.TOL
    assert big.sum() > B // 2 and np.all(gv[6:9, big] == 0.0)
    errs = dict(vec=rel(gv, ob.vec[:n]), quat=rel(gq, ob.quat), cov=rel(gP, ob.cov[:n, :n]), ll=rel(gll, ob.ll))
    assert max(errs.values()) < 1e-9, errs
