"""pd_xolp_stats / polardepth.polar.XolpStats on the GPU against NumPy on the very tensor handed to the kernel.

The reference: the header's bin formulas in np.float32, math.fsum (exact) for the four sums, ndarray.mean() / .std() in fp64
for the derived values.  Integer fields and extrema must match exactly.  The sums: any summation order of N exactly
converted terms errs by at most (N - 1) 2^-53 sum|x|, so the tests assert |got - exact| <= N 2^-53 sum|x| per sum.  The
derived mean / std: 1e-9 relative -- forming the variance as sum(x^2) / n - mean^2 amplifies the sum error by
1 + mean^2 / var, the inputs keep that factor <= 10 for both channels (asserted), and with N <= 2^19 the bound is ~6e-10."""
import functools
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

C1, C2 = np.float32(np.pi / 2), np.float32(256 / np.pi)
# (B, H, W, ld): a single quad | a partial last quad and padding columns | several workgroups (2 of 1024 lanes) | the
# production pitch: 78336 quads, which the kernel spreads over 20 workgroups of 1024 lanes, about four grid strides each
# (it takes one workgroup per 4096 quads up to its cap of 256, so every lane walks the strided loop with its carries; the cap
# itself is NOT reached by these four: test_the_capped_grid_at_production_size below runs 256 workgroups)
CASES = [(1, 1, 4, 4), (2, 5, 10, 12), (3, 64, 96, 96), (2, 256, 612, 640)]
INT_KEYS = ("n", "nonfinite", "over_diffuse", "over_one")
EXT_KEYS = ("dolp_min", "dolp_max", "aolp_min", "aolp_max")
DERIVED = ("dolp_mean", "dolp_std", "aolp_mean", "aolp_std", "xolp_mean", "xolp_std")


def _thresholds():
    from polardepth import polar
    return np.float32(polar.theta_tables_numpy(1.5)[0][0].max()), np.float32(1.0)


def included(x, W, mask=None):
    """x [B,2,H,ld] float32, mask [B,H,ld] or None -> (rho, phi) of the included pixels (float32, 1-D), nonfinite count."""
    rho, phi = x[:, 0, :, :W], x[:, 1, :, :W]
    passes = np.ones(rho.shape, bool) if mask is None else mask[:, :, :W] != 0
    fin = np.isfinite(rho) & np.isfinite(phi)
    return rho[passes & fin], phi[passes & fin], int((passes & ~fin).sum())


def ref_of_values(r, p, nonfinite=0):
    """The reference record of included values r, p (float32, 1-D)."""
    t0, t1 = _thresholds()
    with np.errstate(over="ignore", invalid="ignore"):
        kr = np.where(r < 0, 0, np.where(r >= 1, 256, (r * np.float32(256.0)).astype(np.int64)))
        t = (p + C1) * C2
        assert t.dtype == np.float32
        kp = np.where(t < 0, 0, np.where(t >= 256, 255, t.astype(np.int64)))
    r64, p64 = r.astype(np.float64), p.astype(np.float64)
    out = {
        "n": int(r.size), "nonfinite": int(nonfinite), "over_diffuse": int((r > t0).sum()), "over_one": int((r > t1).sum()),
        "sums": [math.fsum(r64), math.fsum(r64 * r64), math.fsum(p64), math.fsum(p64 * p64)],
        "abs": [float(np.abs(r64).sum()), float((r64 * r64).sum()), float(np.abs(p64).sum()), float((p64 * p64).sum())],
        "hist_dolp": np.bincount(kr, minlength=257).astype(np.uint64),
        "hist_aolp": np.bincount(kp, minlength=256).astype(np.uint64),
        "dolp_min": r.min() if r.size else np.inf, "dolp_max": r.max() if r.size else -np.inf,
        "aolp_min": p.min() if p.size else np.inf, "aolp_max": p.max() if p.size else -np.inf,
    }
    if r.size:
        out.update(dolp_mean=r64.mean(), dolp_std=r64.std(), aolp_mean=p64.mean(), aolp_std=p64.std())
        out.update(xolp_mean=0.5 * (out["dolp_mean"] + out["aolp_mean"]), xolp_std=0.5 * (out["dolp_std"] + out["aolp_std"]))
        out["amplification"] = max(1 + out["dolp_mean"] ** 2 / out["dolp_std"] ** 2 if out["dolp_std"] else np.inf,
                                   1 + out["aolp_mean"] ** 2 / out["aolp_std"] ** 2 if out["aolp_std"] else np.inf)
    return out


def check(got, ref, derived=True, what=""):
    for k in INT_KEYS:
        print(what, k, got[k], ref[k])
        assert got[k] == ref[k], (what, k)
    for k in EXT_KEYS:
        print(what, k, got[k], ref[k])
        assert got[k] == ref[k], (what, k)
    assert np.array_equal(got["hist_dolp"], ref["hist_dolp"]), what
    assert np.array_equal(got["hist_aolp"], ref["hist_aolp"]), what
    assert int(got["hist_dolp"].sum()) == int(got["hist_aolp"].sum()) == ref["n"]
    N = ref["n"]
    for i in range(4):
        err, bound = abs(float(got["sums"][i]) - ref["sums"][i]), N * 2.0 ** -53 * ref["abs"][i]
        print(what, "sum", i, "err", err, "bound", bound)
        assert err <= bound, (what, i, err, bound)
    if N == 0:
        assert all(math.isnan(got[k]) for k in DERIVED) and math.isnan(got["frac_over_diffuse"]) and math.isnan(got["frac_over_one"])
        return
    assert got["frac_over_diffuse"] == ref["over_diffuse"] / N and got["frac_over_one"] == ref["over_one"] / N
    if derived:
        assert N <= 2 ** 19
        print(what, "amplification", ref["amplification"])
        assert ref["amplification"] <= 10, (what, ref["amplification"])
        for k in DERIVED:
            print(what, k, got[k], ref[k])
            assert abs(got[k] - ref[k]) <= 1e-9 * abs(ref[k]), (what, k, got[k], ref[k])


@functools.lru_cache(maxsize=None)
def iid_case(case):
    """An i.i.d. tensor of the case's shape (host, read-only): DoLP uniform in [-0.05, 1.25), AoLP a little beyond +-pi/2; the
    padding columns hold NaN and 1e30, which must not be seen.  Returns (x, reference without a mask)."""
    B, H, W, ld = case
    rng = np.random.default_rng(1000 + B * H * W)
    x = np.empty((B, 2, H, ld), np.float32)
    x[:, 0] = rng.uniform(-0.05, 1.25, (B, H, ld))
    x[:, 1] = rng.uniform(-1.6, 1.6, (B, H, ld))
    x[:, 0, :, W:] = np.nan
    x[:, 1, :, W:] = 1e30
    x.setflags(write=False)
    return x, ref_of_values(*included(x, W))


@functools.lru_cache(maxsize=None)
def smooth_case(general):
    """K1's own output on the planes of two synthetic items, 256 x 612 -> pitch 640 (LUT kernel, or the general kernel with
    angles=): (device tensor, width, reference)."""
    from polardepth import polar, synthetic
    pol = synthetic.make_batch(2, 256, 612, frame_w=612, device="cuda", seed=11)[("pol", 0, 0)]
    kw = {"angles": np.array([2.0, 43.5, 91.0, 133.0]) * np.pi / 180} if general else {}
    x = polar.polar_forward(pol, want=("xolp",), out_width=640, **kw)["xolp"]
    return x, 612, ref_of_values(*included(x.cpu().numpy(), 612))


@pytest.mark.parametrize("case", CASES, ids=lambda c: "x".join(map(str, c)))
def test_iid_tensor_matches_numpy(case):
    from polardepth import polar
    x, ref = iid_case(case)
    got = polar.xolp_stats(torch.from_numpy(x.copy()).cuda(), width=case[2])
    assert got["thresholds"] == tuple(float(t) for t in _thresholds())
    check(got, ref, what=str(case))


@pytest.mark.parametrize("general", [False, True], ids=["lut", "general"])
def test_realistic_maps_match_numpy(general):
    from polardepth import polar
    x, W, ref = smooth_case(general)
    assert ref["n"] == 2 * 256 * 612 and ref["nonfinite"] == 0
    check(polar.xolp_stats(x, width=W), ref, what="smooth")


def test_constant_runs_take_the_aggregated_histogram_path():
    """Piecewise-constant maps (a saturated or black region, a zero-filled frame): quads that hold one bin, in runs of lanes
    that start and end anywhere in a wave and cross rows, interrupted by masked and non-finite pixels -- the case in which
    only the first lane of a run adds to the workgroup's histogram."""
    from polardepth import polar
    B, H, W = 2, 48, 96
    i = np.arange(B * H * W)
    x = np.empty((B, 2, H, W), np.float32)
    x[:, 0] = (((i // 150) * 37 % 300) / np.float32(256)).astype(np.float32).reshape(B, H, W)      # runs of 37.5 quads
    x[:, 1] = ((((i // 1000) * 29 % 256) - 128 + 0.5) / C2).astype(np.float32).reshape(B, H, W)     # runs of 250 quads
    x[1, 0, 5::97] = np.nan
    mask = np.ones((B, H, W), np.uint8)
    mask.reshape(-1)[3::211] = 0
    ref = ref_of_values(*included(x, W, mask))
    assert np.count_nonzero(ref["hist_dolp"]) > 20 and ref["nonfinite"] > 0
    quads = (np.nan_to_num(x[:, 0]).reshape(-1, 4) * np.float32(256)).astype(np.int64)
    assert 0.9 < (quads == quads[:, :1]).all(1).mean() < 1
    check(polar.xolp_stats(torch.from_numpy(x).cuda(), mask=torch.from_numpy(mask).cuda()), ref, derived=False, what="runs")
    x[:] = 0                                        # one bin for everything: a single add per wave and channel
    got = polar.xolp_stats(torch.from_numpy(x).cuda())
    assert got["hist_dolp"][0] == got["hist_aolp"][128] == got["n"] == B * H * W and got["dolp_std"] == 0.0


def adversarial():
    t0 = _thresholds()[0]
    one = np.float32(1)
    rho = [np.float32(k / 256) for k in range(257)]
    rho += [np.nextafter(one, np.float32(0)), one, np.nextafter(one, np.float32(2)), np.float32(2.2), np.float32(-0.25),
            np.float32(-0.0), np.float32(-1e-45), t0, np.nextafter(t0, one), np.nextafter(t0, np.float32(0)),
            np.float32(3e38), np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    phi = [-C1, C1, np.float32(0), np.nextafter(C1, np.float32(0)), np.nextafter(-C1, np.float32(0)),
           np.nextafter(C1, np.float32(2)), np.nextafter(-C1, np.float32(-2)), np.float32(1.6), np.float32(-1.6),
           np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf)]
    assert len(phi) % 4 == 0
    x = np.empty((1, 2, len(rho), len(phi)), np.float32)
    x[0, 0] = np.array(rho, np.float32)[:, None]
    x[0, 1] = np.array(phi, np.float32)[None, :]
    return x, rho, phi


def test_adversarial_table_bins_and_counters_are_exact():
    """Every bin edge, the threshold itself (strictly greater), -0.0, values beyond both ranges and non-finite values in
    either channel, against a scalar restatement of the header (and against the vectorised reference)."""
    from polardepth import polar
    x, rho, phi = adversarial()
    t0, t1 = _thresholds()
    hd, ha = np.zeros(257, np.uint64), np.zeros(256, np.uint64)
    n = nonfinite = over0 = over1 = 0
    for r in rho:
        for p in phi:
            if not (np.isfinite(r) and np.isfinite(p)):
                nonfinite += 1
                continue
            n += 1
            over0 += bool(r > t0)
            over1 += bool(r > t1)
            hd[0 if r < 0 else (256 if r >= 1 else int(np.float32(r * np.float32(256.0))))] += 1
            t = np.float32(np.float32(p + C1) * C2)
            ha[0 if t < 0 else (255 if t >= 256 else int(t))] += 1
    got = polar.xolp_stats(torch.from_numpy(x).cuda())
    assert (got["n"], got["nonfinite"], got["over_diffuse"], got["over_one"]) == (n, nonfinite, over0, over1)
    assert np.array_equal(got["hist_dolp"], hd) and np.array_equal(got["hist_aolp"], ha)
    fin_phi = sum(bool(np.isfinite(p)) for p in phi)
    assert got["hist_dolp"][1] == fin_phi and got["hist_dolp"][255] == 2 * fin_phi          # 255/256 and nextafter(1, 0)
    assert got["hist_dolp"][256] == 5 * fin_phi                                             # 256/256, 1.0, its successor, 2.2, 3e38
    assert got["hist_dolp"][0] == 4 * fin_phi                                               # 0, -0.25, -0.0, the negative denormal
    assert got["over_one"] == 3 * fin_phi and got["over_diffuse"] > got["over_one"]
    assert (got["dolp_min"], got["dolp_max"]) == (-0.25, float(np.float32(3e38)))
    assert (got["aolp_min"], got["aolp_max"]) == (float(np.float32(-1.6)), float(np.float32(1.6)))
    check(got, ref_of_values(*included(x, x.shape[3])), derived=False, what="adversarial")


def test_masks_of_three_dtypes_and_the_empty_selection():
    from polardepth import polar
    case = CASES[2]
    x, _ = iid_case(case)
    B, H, W, ld = case
    half = np.random.default_rng(5).random((B, 1, H, ld)) < 0.5
    ref = ref_of_values(*included(x, W, half[:, 0]))
    xd = torch.from_numpy(x.copy()).cuda()
    records = []
    for m in (torch.from_numpy(half), torch.from_numpy(half.astype(np.uint8) * 255), torch.from_numpy(half.astype(np.int32) * 20)):
        st = polar.XolpStats("cuda").add(xd, width=W, mask=m.cuda())
        check(st.result(), ref, what=str(m.dtype))
        records.append(st._record.clone())
    assert torch.equal(records[0], records[1]) and torch.equal(records[0], records[2])
    check(polar.xolp_stats(xd, width=W, mask=torch.from_numpy(half[:, 0]).cuda()), ref, what="[B,H,W]")
    # a non-finite pixel behind a zero mask is not even counted as non-finite
    y = x.copy()
    y[:, 0][~half[:, 0]] = np.nan
    got = polar.xolp_stats(torch.from_numpy(y).cuda(), width=W, mask=torch.from_numpy(half).cuda())
    assert got["nonfinite"] == 0
    check(got, ref, what="nan behind the mask")
    # nothing selected: n == 0, extrema +-inf, NaN means without raising
    got = polar.xolp_stats(xd, width=W, mask=torch.zeros((B, 1, H, ld), dtype=torch.bool, device="cuda"))
    assert got["n"] == 0 and got["nonfinite"] == 0
    assert (got["dolp_min"], got["dolp_max"], got["aolp_min"], got["aolp_max"]) == (math.inf, -math.inf, math.inf, -math.inf)
    check(got, ref_of_values(np.empty(0, np.float32), np.empty(0, np.float32)), what="empty")
    with pytest.raises(ValueError, match="mask must be"):
        polar.xolp_stats(xd, mask=torch.zeros((B, H, ld - 4), dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="mask must be"):
        polar.xolp_stats(xd, mask=torch.zeros((B, H, ld), dtype=torch.float32, device="cuda"))


def test_empty_batch_and_argument_errors():
    from polardepth import polar
    st = polar.XolpStats("cuda")
    st._record.fill_(0xAB)
    st.reset()                                  # pd_xolp_stats with B == 0 and accumulate == 0 writes the empty record
    empty = ref_of_values(np.empty(0, np.float32), np.empty(0, np.float32))
    check(st.result(), empty, what="reset")
    check(polar.xolp_stats(torch.empty((0, 2, 8, 8), device="cuda")), empty, what="B == 0")
    x, ref = iid_case(CASES[1])
    st.add(torch.from_numpy(x.copy()).cuda(), width=CASES[1][2])
    before = st._record.clone()
    st.add(torch.empty((0, 2, 8, 8), device="cuda"))              # adds nothing
    assert torch.equal(before, st._record)
    check(st.result(), ref, what="after the empty add")
    for bad in (torch.zeros((2, 3, 8, 8)), torch.zeros((2, 8, 8)), torch.zeros((2, 2, 8, 8), dtype=torch.float64),
                torch.zeros((2, 2, 8, 8), dtype=torch.float16)):
        with pytest.raises(ValueError, match="float32"):
            st.add(bad.cuda())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        st.add(torch.zeros((2, 2, 8, 8)))
    with pytest.raises(RuntimeError, match="multiple of 4"):
        st.add(torch.zeros((1, 2, 4, 6), device="cuda"))
    with pytest.raises(RuntimeError, match="exceeds the row pitch"):
        st.add(torch.zeros((1, 2, 4, 8), device="cuda"), width=9)


@pytest.mark.parametrize("kind", ["smooth", "iid"])
def test_the_record_is_bit_reproducible(kind):
    from polardepth import polar
    if kind == "smooth":
        x, W, _ = smooth_case(False)
    else:
        x, W = torch.from_numpy(iid_case(CASES[3])[0].copy()).cuda(), CASES[3][2]
    a = polar.XolpStats("cuda").add(x, width=W)._record.clone()
    b = polar.XolpStats("cuda").add(x, width=W)._record.clone()
    st = polar.XolpStats("cuda").add(x[:1], width=W)
    st.reset()
    c = st.add(x, width=W)._record.clone()
    assert torch.equal(a, b) and torch.equal(a, c)
    assert int.from_bytes(bytes(a[:8].cpu().tolist()), "little") == x.shape[0] * x.shape[2] * W


def test_accumulation_equals_numpy_over_the_concatenation():
    from polardepth import polar
    parts = [iid_case(CASES[2]), iid_case(CASES[1]), iid_case(CASES[0])]
    st = polar.XolpStats("cuda")
    rs, ps = [], []
    for (x, _), case in zip(parts, (CASES[2], CASES[1], CASES[0])):
        st.add(torch.from_numpy(x.copy()).cuda(), width=case[2])
        r, p, _ = included(x, case[2])
        rs.append(r); ps.append(p)
    check(st.result(), ref_of_values(np.concatenate(rs), np.concatenate(ps)), what="A + B + C")
    st.reset()
    check(st.result(), ref_of_values(np.empty(0, np.float32), np.empty(0, np.float32)), what="reset")
    st.add(torch.from_numpy(parts[1][0].copy()).cuda(), width=CASES[1][2])
    check(st.result(), parts[1][1], what="after reset")


def test_the_capped_grid_at_production_size():
    """13 x 512 x 638 (pitch 640): 1 064 960 quads, past the 256 x 4096 the kernel's grid is capped at, so 256 workgroups walk
    a little over four strides per lane -- the regime of a production batch.  Integer fields, extrema and histograms exactly;
    the record twice, byte for byte.  math.fsum over 4 million values would take seconds, so the sums are held against NumPy's
    sum in x87 extended precision (64-bit significand): that reference errs by at most N 2^-64 sum|x| itself, which is added to
    the bound N 2^-53 sum|x| of the other tests."""
    from polardepth import polar
    assert np.finfo(np.longdouble).nmant >= 63, "this test needs an extended-precision long double (x86)"
    B, H, W, ld = 13, 512, 638, 640
    rng = np.random.default_rng(77)
    x = np.empty((B, 2, H, ld), np.float32)
    x[:, 0] = rng.random((B, H, ld), dtype=np.float32) * np.float32(1.3) - np.float32(0.05)
    x[:, 1] = (rng.random((B, H, ld), dtype=np.float32) - np.float32(0.5)) * np.float32(3.2)
    x[:, :, :, W:] = np.nan
    r, p, nonfinite = included(x, W)
    t0, t1 = _thresholds()
    xd = torch.from_numpy(x).cuda()
    st = polar.XolpStats("cuda").add(xd, width=W)
    got, first = st.result(), st._record.clone()
    assert torch.equal(first, polar.XolpStats("cuda").add(xd, width=W)._record)
    N = B * H * W
    assert (got["n"], got["nonfinite"], got["over_diffuse"], got["over_one"]) == (N, 0, int((r > t0).sum()), int((r > t1).sum()))
    assert (got["dolp_min"], got["dolp_max"], got["aolp_min"], got["aolp_max"]) == (r.min(), r.max(), p.min(), p.max())
    kr = np.where(r < 0, 0, np.where(r >= 1, 256, (r * np.float32(256.0)).astype(np.int64)))
    kp = np.clip(((p + C1) * C2).astype(np.int64), None, 255)
    kp[(p + C1) * C2 < 0] = 0
    assert np.array_equal(got["hist_dolp"], np.bincount(kr, minlength=257)) and np.array_equal(got["hist_aolp"], np.bincount(kp, minlength=256))
    for i, v in enumerate((r, r, p, p)):
        v = v.astype(np.longdouble)
        terms = v * v if i % 2 else v                      # exact: 48 bits fit the 64-bit significand
        ref, mag = terms.sum(), np.abs(terms).sum()
        err, bound = abs(np.longdouble(got["sums"][i]) - ref), N * (2.0 ** -53 + 2.0 ** -64) * mag
        print("capped sum", i, "err", float(err), "bound", float(bound))
        assert err <= bound, (i, float(err), float(bound))
