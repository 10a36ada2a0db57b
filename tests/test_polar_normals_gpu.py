"""pd_polar_normals_stats / polardepth.polar_normals_eval on the GPU against the NumPy statement (tests/polar_normals_ref.py,
pinned by tests/test_polar_normals_ref.py) applied to the very arrays handed to the kernel.

n, every counter, both histograms, choice and the NaN / zero patterns of the maps must be equal; pol_normal bit-equal.  The
eight sums: rtol 1e-11, the bar tests/test_normals_stats_gpu.py derives for this reducer -- any order of n exactly converted
terms errs by at most (n - 1) 2^-53 of the sum, 2.3e-13 at the 2080 pixels of the largest image here; the device acos adds a
few ulp per term.  The degree maps: atol 1e-5 degrees (they are stored as fp32: half an ulp at 180 degrees is 7.6e-6)."""
import functools
import math

import numpy as np
import pytest
import torch

import polar_normals_ref as R

pytestmark = pytest.mark.gpu

# (N, H, W, ldp, ld): less than a wave | padded rows, both pixel strides | 2080 pixels: more than one workgroup per image
SHAPES = [(1, 1, 4, 4, 3), (2, 5, 20, 24, 3), (2, 5, 20, 24, 4), (3, 40, 52, 52, 4)]
TILT_DEG = 5.0
TILT2 = math.sin(math.radians(TILT_DEG)) ** 2


def PE():
    from polardepth import polar_normals_eval
    return polar_normals_eval


def _classes(K):
    from polardepth import normals_eval
    return [("all", None)] if K == 1 else list(normals_eval.DEFAULT_CLASSES)


def _lohi(classes):
    return [(1, 0) if r is None else tuple(r) for _, r in classes]


def _edges():
    from polardepth import normals_eval
    return normals_eval.cos_edges_numpy()


@functools.lru_cache(maxsize=None)
def case(N, H, W, ldp, ld):
    c = R.random_case(100 * N + H + W + ld, N, H, W, ldp, ld, masked=True)
    for a in c.values():
        a.setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(shape, K, sign=1):
    """The statement on a case, computed once and shared (never modified)."""
    c = case(*shape)
    return R.stats(c["pred"], c["pol"], c["xolp"], c["mask"] if K > 1 else None, _lohi(_classes(K)), _edges(), valid=c["valid"],
                   tilt2_min=TILT2, aolp_sign=sign)


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()                 # a writable copy: the case arrays are read-only


def tensors(shape, K):
    """The case on the device as the Python layer takes it: pred an [N,3,H,W] view of pixel stride ld, pol_normals and xolp
    views of row pitch ldp."""
    N, H, W, ldp, ld = shape
    c = case(*shape)
    pred = _dev(c["pred"]).permute(0, 3, 1, 2)[:, :3]
    pol, xolp = _dev(c["pol"])[..., :W], _dev(c["xolp"])[..., :W]
    mask = _dev(c["mask"])[:, None] if K > 1 else None
    return pred, pol, xolp, mask, _dev(c["valid"])[:, None]


def run(shape, K, sign=1, maps=True):
    pred, pol, xolp, mask, valid = tensors(shape, K)
    return PE().polar_normals_stats(pred, pol, xolp, mask=mask, valid=valid, classes=_classes(K), tilt_min_deg=TILT_DEG,
                                    aolp_sign=sign, maps=maps)


def fields(st):
    torch.cuda.synchronize()
    out = {}
    for name, rs in (("normal", st.normal), ("azimuth", st.azimuth)):
        out[name] = {"n": rs.n.cpu().numpy(), "sums": rs.sums.cpu().numpy(), "hist": rs.hist.cpu().numpy().astype(np.int64)}
        for c in rs.counter_names:
            out[name][c] = getattr(rs, c).cpu().numpy()
    for m in ("az_deg", "n_deg", "choice", "pol_normal"):
        out[m] = None if getattr(st, m) is None else getattr(st, m).cpu().numpy()
    return out


def compare(got, ref, what, sets=("normal", "azimuth")):
    for name in sets:
        for k in ref[name]:
            if k == "sums":
                rel = np.abs(got[name][k] - ref[name][k]) / np.maximum(np.abs(ref[name][k]), 1e-300)
                print(what, name, "sums: max rel err", rel.max())
                assert np.allclose(got[name][k], ref[name][k], rtol=1e-11, atol=0.0), (what, name, rel.max())
            else:
                assert np.array_equal(got[name][k], ref[name][k]), (what, name, k)
    if got["choice"] is not None:
        assert np.array_equal(got["choice"], ref["choice"]), what
        assert np.array_equal(got["pol_normal"].view(np.int32), ref["pol_normal"].view(np.int32)), what
    for m in ("az_deg", "n_deg"):
        if got[m] is None:
            continue
        assert np.array_equal(np.isnan(got[m]), np.isnan(ref[m])), (what, m)
        ok = ~np.isnan(ref[m])
        d = np.abs(got[m][ok].astype(np.float64) - ref[m][ok])
        print(what, m, "max abs err", d.max() if d.size else 0.0)
        assert (d <= 1e-5).all(), (what, m, d.max())


def test_the_cases_reach_every_counter_and_choice():
    """Asserted on the statement, before anything runs on the device.  The four pixels of the smallest case cannot show ten
    events; every other case must, on its own."""
    for shape in SHAPES[1:]:
        ref = reference(shape, 12)
        for name, counters in (("normal", R.NORMAL_COUNTERS), ("azimuth", R.AZIMUTH_COUNTERS)):
            for c in counters:
                assert ref[name][c][:, 0].sum() > 0, (shape, name, c)
            assert ref[name]["n"][:, 0].sum() > 0
        assert set(np.unique(ref["choice"])) == set(range(7)), shape
        assert (ref["normal"]["n"][:, 1:].sum(0) > 0).all()                 # every material has pixels
    assert reference(SHAPES[0], 1)["normal"]["n"].sum() > 0


@pytest.mark.parametrize("K", [1, 12])
@pytest.mark.parametrize("shape", SHAPES)
def test_records_and_maps_equal_the_statement(shape, K):
    pe = PE()
    N, H, W, ldp, ld = shape
    pred, pol, xolp, mask, valid = tensors(shape, K)
    if H > 1:
        assert pe._row_pitch(pol, 9, H, W) == ldp == pe._row_pitch(xolp, 2, H, W)      # read in place, padding and all
    st = run(shape, K)
    assert st.names == [n for n, _ in _classes(K)]
    assert tuple(st.normal.records.shape) == (N, K, pe.NORMAL_RECORD_BYTES)
    assert tuple(st.azimuth.records.shape) == (N, K, pe.AZIMUTH_RECORD_BYTES)
    compare(fields(st), reference(shape, K), (shape, K))


def test_aolp_sign_and_contiguous_inputs():
    shape = SHAPES[2]
    compare(fields(run(shape, 12, sign=-1)), reference(shape, 12, -1), "aolp_sign = -1")
    pred, pol, xolp, mask, valid = tensors(shape, 12)
    st = PE().polar_normals_stats(pred.contiguous(), pol.contiguous(), xolp.contiguous(), mask=mask, valid=valid,
                                  tilt_min_deg=TILT_DEG, maps=True)
    compare(fields(st), reference(shape, 12), "contiguous copies")


def test_either_record_set_may_be_null():
    """Through the C ABI: the other set and its maps are as in the full call; a NULL set with its maps asked for still writes them."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    from polardepth import normals_eval as ne
    pe = PE()
    shape = SHAPES[3]
    N, H, W, ldp, ld = shape
    full = run(shape, 12)
    pred, pol, xolp, mask, valid = tensors(shape, 12)
    names, table = ne.class_table(_classes(12))
    pred_pm, ld_pm = ne.pixel_major(pred)
    assert ld_pm == ld
    mask_i, valid_u = mask[:, 0].contiguous(), valid[:, 0].contiguous()
    ws = torch.empty(int(lib.pd_polar_normals_stats_workspace(N, H, W, 12)), dtype=torch.uint8, device="cuda")
    for which in ("normal", "azimuth"):
        rec = torch.full_like(getattr(full, which).records, 0x5A)
        az, nd = torch.full((N, H, W), 7.0, device="cuda"), torch.full((N, H, W), 7.0, device="cuda")
        ch, pn = torch.full((N, H, W), 9, dtype=torch.uint8, device="cuda"), torch.full((N, H, W, 4), 7.0, device="cuda")
        check(lib.pd_polar_normals_stats(ptr(pred_pm), ld, ptr(pol), ptr(xolp), ldp, ptr(mask_i), table, 12, ptr(valid_u),
                                         ptr(ne.cos_edges("cuda")), 0.05, 1.0, TILT2, 1,
                                         ptr(rec) if which == "normal" else None, ptr(rec) if which == "azimuth" else None,
                                         ptr(az), ptr(nd), ptr(ch), ptr(pn), ptr(ws), ws.numel(), N, H, W, stream_ptr()), which)
        torch.cuda.synchronize()
        assert torch.equal(rec, getattr(full, which).records), which
        assert az.cpu().numpy().tobytes() == full.az_deg.cpu().numpy().tobytes()
        assert nd.cpu().numpy().tobytes() == full.n_deg.cpu().numpy().tobytes()
        assert torch.equal(ch, full.choice) and pn.cpu().numpy().tobytes() == full.pol_normal.cpu().numpy().tobytes()
    # records only, no map
    plain = run(shape, 12, maps=False)
    assert plain.az_deg is None and plain.pol_normal is None
    assert torch.equal(plain.normal.records, full.normal.records) and torch.equal(plain.azimuth.records, full.azimuth.records)


def test_an_empty_batch():
    pe = PE()
    z = lambda c: torch.zeros((0, c, 6, 8), device="cuda")
    st = pe.polar_normals_stats(z(3), z(9), z(2), classes=[("all", None)], maps=True)
    assert tuple(st.normal.records.shape) == (0, 1, pe.NORMAL_RECORD_BYTES) and tuple(st.az_deg.shape) == (0, 6, 8)
    assert tuple(st.azimuth.pooled().shape) == (1, 8)
    # the C call itself: PD_OK, and nothing is written
    from polardepth._lib import lib, ptr, stream_ptr
    from polardepth import normals_eval as ne
    names, table = ne.class_table([("all", None)])
    buf = torch.full((4096,), 0x5A, dtype=torch.uint8, device="cuda")
    rc = lib.pd_polar_normals_stats(ptr(buf), 4, ptr(buf), ptr(buf), 8, None, table, 1, None, ptr(ne.cos_edges("cuda")), 0.05, 1.0,
                                    0.0, 1, ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(buf), ptr(buf), buf.numel(),
                                    0, 6, 8, stream_ptr())
    torch.cuda.synchronize()
    assert rc == 0 and bool((buf == 0x5A).all())


def test_no_mask_needs_unranged_classes():
    from polardepth._lib import PolarDepthError
    pred, pol, xolp, mask, valid = tensors(SHAPES[1], 1)
    with pytest.raises(PolarDepthError, match="mask is null"):
        PE().polar_normals_stats(pred, pol, xolp)                      # the default classes need the mask


def test_two_calls_give_identical_bytes():
    shape = SHAPES[3]
    a = run(shape, 12)
    junk = torch.full((1 << 20,), 0x5A, dtype=torch.uint8, device="cuda")      # whatever the allocator hands out next is dirty
    del junk
    b = run(shape, 12)
    torch.cuda.synchronize()
    for x, y in ((a.normal.records, b.normal.records), (a.azimuth.records, b.azimuth.records), (a.az_deg, b.az_deg),
                 (a.n_deg, b.n_deg), (a.choice, b.choice), (a.pol_normal, b.pol_normal)):
        assert x.cpu().numpy().tobytes() == y.cpu().numpy().tobytes()


def test_captured_call_replays_the_eager_bytes():
    pe = PE()
    shape = SHAPES[3]
    pred, pol, xolp, mask, valid = tensors(shape, 12)
    kw = dict(mask=mask, valid=valid, tilt_min_deg=TILT_DEG, maps=True)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                       # warm-up on a side stream, as stream capture requires (builds the table)
        eager = pe.polar_normals_stats(pred, pol, xolp, **kw)
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                       # one stream: no parallel branches
        st = pe.polar_normals_stats(pred, pol, xolp, **kw)
    st.normal.records.zero_()
    st.azimuth.records.zero_()
    st.choice.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(st.normal.records, eager.normal.records) and torch.equal(st.azimuth.records, eager.azimuth.records)
    assert torch.equal(st.choice, eager.choice)
    assert st.pol_normal.cpu().numpy().tobytes() == eager.pol_normal.cpu().numpy().tobytes()
    assert st.az_deg.cpu().numpy().tobytes() == eager.az_deg.cpu().numpy().tobytes()
    assert st.n_deg.cpu().numpy().tobytes() == eager.n_deg.cpu().numpy().tobytes()


def _np_metrics(r):
    """METRIC_NAMES from the statement's fields, in NumPy: n [...], sums [..., 4], hist [..., bins]."""
    n, sums, hist = r["n"].astype(np.float64), r["sums"], r["hist"]
    cs = hist.cumsum(-1)
    with np.errstate(all="ignore"):
        half = n / 2
        b = np.minimum((cs < half[..., None]).sum(-1), hist.shape[-1] - 1)
        hb = np.take_along_axis(hist, b[..., None], -1)[..., 0]
        below = np.take_along_axis(cs, b[..., None], -1)[..., 0] - hb
        median = (b + (half - below) / hb) * 0.25
        share = lambda k: cs[..., k - 1] / n
        return np.stack([sums[..., 0] / n, median, np.sqrt(sums[..., 1] / n), share(45), share(90), share(120), n,
                         sums[..., 2] / sums[..., 3]], -1)


def test_metrics_and_pool_follow_the_fields():
    shape = SHAPES[3]
    ref = reference(shape, 12)
    st = run(shape, 12)
    for name, rs in (("normal", st.normal), ("azimuth", st.azimuth)):
        r = ref[name]
        m = rs.metrics()
        assert m.is_cuda and m.dtype == torch.float64 and tuple(m.shape) == (shape[0], 12, 8)
        assert np.allclose(m.cpu().numpy(), _np_metrics(r), rtol=1e-9, atol=0.0, equal_nan=True)
        deg = ref["n_deg" if name == "normal" else "az_deg"][0]
        live = case(*shape)["valid"][0] != 0
        deg = deg[~np.isnan(deg) & live]                                          # class "all" of image 0
        got = m[0, 0].cpu().numpy()
        assert got[6] == deg.size and abs(got[1] - np.median(deg)) <= 0.25 and got[3] == (deg < 11.25).sum() / deg.size
        tot = {k: v.sum(0) for k, v in r.items()}
        assert np.allclose(rs.pooled().cpu().numpy(), _np_metrics(tot), rtol=1e-9, atol=0.0, equal_nan=True)
        want = np.stack([tot[c] for c in rs.counter_names], -1)
        assert np.array_equal(rs.pooled_counters().cpu().numpy(), want)
    st += run(shape, 12)                                                           # pools both sets on the device
    for name, rs in (("normal", st.normal), ("azimuth", st.azimuth)):
        tot = {k: 2 * v.sum(0) for k, v in ref[name].items()}
        twice = rs.pooled().cpu().numpy()
        assert np.array_equal(twice[:, 6], tot["n"]) and np.allclose(twice, _np_metrics(tot), rtol=1e-9, equal_nan=True)
        assert np.array_equal(rs.pooled_counters().cpu().numpy(), np.stack([tot[c] for c in rs.counter_names], -1))
    with pytest.raises(ValueError, match="cannot pool"):
        st += run(shape, 1)


def test_a_depth_map_scores_as_its_own_normals():
    from polardepth._lib import lib, check, ptr, stream_ptr
    shape = SHAPES[3]
    N, H, W, ldp, ld = shape
    pred, pol, xolp, mask, valid = tensors(shape, 12)
    rng = np.random.default_rng(5)
    depth = _dev((1.0 + 0.1 * rng.random((N, 1, H, W))).astype(np.float32))
    Km = torch.eye(4, device="cuda")[None].repeat(N, 1, 1)
    Km[:, 0, 0], Km[:, 1, 1], Km[:, 0, 2], Km[:, 1, 2] = 0.58 * W, 1.92 * H, 0.5 * W, 0.5 * H
    a = PE().polar_normals_stats(depth, pol, xolp, K=Km, mask=mask, valid=valid, tilt_min_deg=TILT_DEG)
    pn = torch.empty((N, H, W, 4), device="cuda")
    big = float(np.finfo(np.float32).max)
    check(lib.pd_gt_normals(ptr(depth), ptr(Km), ptr(pn), N, H, W, -big, big, stream_ptr()), "pd_gt_normals")
    b = PE().polar_normals_stats(pn.permute(0, 3, 1, 2)[:, :3], pol, xolp, mask=mask, valid=valid, tilt_min_deg=TILT_DEG)
    assert torch.equal(a.normal.records, b.normal.records) and torch.equal(a.azimuth.records, b.azimuth.records)
    c = case(*shape)
    ref = R.stats(pn.cpu().numpy(), c["pol"], c["xolp"], c["mask"], _lohi(_classes(12)), _edges(), valid=c["valid"], tilt2_min=TILT2)
    got = fields(a)
    compare(got, ref, "depth map")
    with pytest.raises(ValueError, match="intrinsics"):
        PE().polar_normals_stats(depth, pol, xolp, mask=mask)
