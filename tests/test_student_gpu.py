"""csrc/student.hip on the device against tests/student_ref.py (NumPy: fp32 per pixel, correctly rounded fp64 sums).

Bounds.  rmask, cmask, lowest_up, minmax, sel, greproj and gmulti are defined operation by operation in fp32 (or are
selections), so they are compared bit for bit.  The three sums add n = N*H*W non-negative terms in fp64 in some fixed order:
against the correctly rounded sum of the same terms the error is at most (n-1) * 2^-53 relative (every partial sum is below
the total, each addition rounds once).  The two float losses are one fp64 division of those sums rounded to fp32: the
reference's quotient differs by far less than half an fp32 ulp, so the roundings differ by at most one ulp.
pd_depth_bins_update is defined operation by operation in fp64: tracker and bins bit for bit.

Shapes (N, h, w, F): (3,2,3,2) is one partly filled wavefront, (3,9,13,2) has a grid-stride tail inside the second
workgroup and two workgroups per item in pd_student_masks, (2,8,16,1) fills whole workgroups with a single frame."""
import numpy as np
import pytest
import torch

import student_ref as S

pytestmark = pytest.mark.gpu

SHAPES = [(3, 2, 3, 2), (3, 9, 13, 2), (2, 8, 16, 1)]
#        motion_masking, avg, aug is NULL, a NaN in mono_depth
MODES = [(1, 0, False, False), (0, 1, False, False), (1, 1, True, False), (1, 0, False, True), (0, 0, True, True)]


def make_inputs(N, h, w, F, nan):
    """Seeded inputs that put at least 5 % of the pixels into every class the kernels distinguish (asserted by the caller)."""
    rng = np.random.default_rng(1000 * N + 100 * h + 10 * w + F)
    H, W = 4 * h, 4 * w
    f32 = np.float32
    depth_q = rng.uniform(0.5, 4.0, (N, h, w)).astype(f32)
    lowest = (f32(1) / depth_q).astype(f32)
    confidence = (rng.random((N, h, w)) > 0.25).astype(f32)
    md = (f32(1) / lowest.repeat(4, 1).repeat(4, 2)).astype(f32)
    cls = rng.random((N, H, W))
    factor = np.where(cls < 0.55, rng.uniform(0.7, 1.4, (N, H, W)),                       # the two depths agree
                      np.where(cls < 0.775, rng.uniform(0.2, 0.45, (N, H, W)),            # (md - t) / t >= 1
                               rng.uniform(2.2, 3.0, (N, H, W)))).astype(f32)             # (t - md) / md >= 1
    mono = (md * factor).astype(f32)
    mono[0, 1, 2] = md[0, 1, 2] * f32(0.5)          # md == 2 t exactly: the first ratio is exactly 1, mask 0
    mono[0, 2, 1] = md[0, 2, 1] * f32(2.0)          # t == 2 md exactly: the second ratio is exactly 1, mask 0
    mono[0, 3, 3] = md[0, 3, 3]                     # equal depths
    confidence[0, 0, 0] = 1                         # ... all of these at a confident pixel
    if nan:
        mono[N - 1, 5, 7] = np.nan
    mono = mono[:, None]
    reproj = [rng.uniform(0.0, 1.0, (N, 1, H, W)).astype(f32) for _ in range(F)]
    if F > 1:
        tie = rng.random((N, 1, H, W)) < 0.2
        reproj[1] = np.where(tie, reproj[0], reproj[1])                                   # a tie between frames
    multi = (mono * rng.uniform(0.8, 1.2, mono.shape)).astype(f32)
    same = rng.random(mono.shape) < 0.1
    multi = np.where(same, mono, multi).astype(f32)                                       # multi == mono: sign 0
    aug = np.zeros(N, f32)
    valid = np.ones((N, F), f32)
    if N == 3:
        aug[1] = 1                                  # item 1 augmented, item 2 without a valid frame
        valid[2] = 0
        if F > 1:
            valid[0, 0] = 0                         # and one missing frame of an otherwise valid item
    else:
        aug[0] = 1                                  # N == 2: item 0 carries both, item 1 neither
        valid[0] = 0
    return dict(lowest=lowest, confidence=confidence, mono=mono, reproj=reproj, multi=multi, aug=aug, valid=valid)


def _cuda(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, want.dtype, got.shape, want.shape)
    same = got == want
    if got.dtype.kind == "f":                                  # a zero's sign counts; any NaN equals any NaN
        same = (same & (np.signbit(got) == np.signbit(want))) | (np.isnan(got) & np.isnan(want))
    assert same.all(), f"{what}: {int((~same).sum())} of {same.size} differ"


def test_inputs_cover_every_class():
    for (N, h, w, F) in SHAPES:
        d = make_inputs(N, h, w, F, nan=False)
        m = S.masks(d["lowest"], d["confidence"], d["mono"], d["aug"], True)
        c = S.combine(d["reproj"], m["rmask"], d["multi"], d["mono"], d["valid"])
        md = (np.float32(1) / m["lowest_up"]).astype(np.float32)
        t = d["mono"][:, 0]
        first = ~(((md - t) / t) < 1)
        second = ~(((t - md) / md) < 1)
        H, W = 4 * h, 4 * w
        share = {"rmask 1": c["r"].mean(), "confidence 0": (~m["conf"]).mean(), "first inequality": first.mean(),
                 "second inequality": second.mean(), "augmented item": (d["aug"] != 0).sum() * H * W / c["r"].size,
                 "no valid frame": (d["valid"].sum(1) == 0).sum() * H * W / c["r"].size}
        print((N, h, w, F), {k: round(float(v), 3) for k, v in share.items()})
        for k, v in share.items():
            assert v >= 0.05, ((N, h, w, F), k, v)
        assert not m["mm"][0, 1, 2] and not m["mm"][0, 2, 1] and m["mm"][0, 3, 3]      # the exact ratios of 1 mask; equality keeps


@pytest.mark.parametrize("mode", MODES, ids=lambda m: "mm%d-avg%d-%s-%s" % (m[0], m[1], "noaug" if m[2] else "aug", "nan" if m[3] else "clean"))
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernels_against_the_numpy_restatement(shape, mode):
    from polardepth import ops
    N, h, w, F = shape
    mm, avg, no_aug, nan = mode
    d = make_inputs(N, h, w, F, nan)
    aug = None if no_aug else d["aug"]
    want = S.masks(d["lowest"], d["confidence"], d["mono"], aug, bool(mm))

    def run():
        rmask, cmask, lowest_up, minmax = ops.student_masks(_cuda(d["lowest"]), _cuda(d["confidence"]), _cuda(d["mono"]),
                                                            None if aug is None else _cuda(aug), motion_masking=bool(mm))
        reproj = [_cuda(r).requires_grad_() for r in d["reproj"]]
        multi = _cuda(d["multi"]).requires_grad_()
        l0, l1, sel, sums = ops.student_combine(reproj, rmask, multi, _cuda(d["mono"]), valid=_cuda(d["valid"]), avg=bool(avg),
                                                details=True)
        (0.75 * l0 + 1.5 * l1).backward()
        torch.cuda.synchronize()
        return {"rmask": rmask, "cmask": cmask, "lowest_up": lowest_up, "minmax": minmax, "sel": sel, "sums": sums,
                "loss": torch.stack([l0, l1]).detach(), "gmulti": multi.grad, **{f"greproj{f}": reproj[f].grad for f in range(F)}}

    got = {k: v.cpu().numpy() for k, v in run().items()}
    for k in ("rmask", "cmask", "lowest_up", "minmax"):
        _same_bits(got[k], want[k], k)
    if nan:
        assert np.isnan(got["minmax"][N - 1]).all() and np.isfinite(got["minmax"][:N - 1]).all()

    c = S.combine(d["reproj"], want["rmask"], d["multi"], d["mono"], d["valid"], avg=bool(avg))
    _same_bits(got["sel"], c["sel"], "sel")
    n = N * 16 * h * w
    for k in range(3):
        err, bound = abs(got["sums"][k] - c["sums"][k]), (n - 1) * 2.0 ** -53 * c["abs_sums"][k]
        print(f"sums[{k}] = {got['sums'][k]!r} want {c['sums'][k]!r} |diff| {err:.3e} bound {bound:.3e}")
        if np.isnan(c["sums"][k]):
            assert np.isnan(got["sums"][k]), k              # the NaN of mono_depth reaches the consistency sum
        else:
            assert err <= bound, (k, err, bound)
    assert got["sums"][1] == c["sums"][1] == c["r"].sum()
    assert np.isnan(c["sums"][2]) == bool(nan) and np.isfinite(c["sums"][:2]).all()
    for k in range(2):
        if np.isnan(c["loss"][k]):
            assert np.isnan(got["loss"][k])
        else:
            ulp = abs(float(got["loss"][k]) - float(c["loss"][k])) / float(np.spacing(abs(c["loss"][k])))
            print(f"loss[{k}] = {got['loss'][k]!r} want {c['loss'][k]!r}: {ulp} ulp")
            assert ulp <= 1.0, (k, ulp)

    greproj, gmulti = S.combine_grad([0.75, 1.5], got["sel"], got["sums"], d["multi"], d["mono"], d["valid"], F, avg=bool(avg))
    for f in range(F):
        _same_bits(got[f"greproj{f}"], greproj[f], f"greproj{f}")
    _same_bits(got["gmulti"], gmulti, "gmulti")
    assert (got["gmulti"] != 0).any() and any((got[f"greproj{f}"] != 0).any() for f in range(F))
    if not no_aug:                                          # an augmented item: no reprojection term anywhere, all consistency
        a = int(np.flatnonzero(d["aug"])[0])
        assert (got["sel"][a] == 255).all() and (got["rmask"][a] == 0).all()
    assert (got["sel"][d["valid"].sum(1) == 0] == 255).all()

    again = {k: v.cpu().numpy() for k, v in run().items()}  # two runs, bit for bit
    for k in got:
        assert got[k].tobytes() == again[k].tobytes(), k


def test_masks_without_the_optional_maps():
    from polardepth import ops
    N, h, w, F = SHAPES[1]
    d = make_inputs(N, h, w, F, nan=False)
    want = S.masks(d["lowest"], d["confidence"], d["mono"], d["aug"], True)
    rmask, cmask, lowest_up, minmax = ops.student_masks(_cuda(d["lowest"]), _cuda(d["confidence"]), _cuda(d["mono"]),
                                                        _cuda(d["aug"]), want_maps=False)
    assert cmask is None and lowest_up is None
    _same_bits(rmask.cpu().numpy(), want["rmask"], "rmask")
    _same_bits(minmax.cpu().numpy(), want["minmax"], "minmax")


@pytest.mark.parametrize("D", [1, 2, 96])
@pytest.mark.parametrize("binning", ["linear", "inverse"])
def test_depth_bins_update_three_steps(binning, D):
    """Tracker and bins bit for bit over three successive updates; the bins are written into the encoder's own depth_bins
    storage, which is what the next plane sweep reads."""
    from polardepth import matching, ops
    from manydepth.networks import ResnetEncoderMatching
    enc = ResnetEncoderMatching(18, False, 32, 48, min_depth_bin=0.1, max_depth_bin=10.0, num_depth_bins=D,
                                depth_binning=binning).cuda()
    storage = enc.depth_bins.data_ptr()
    tracker = torch.tensor([0.1, 10.0], dtype=torch.float64, device="cuda")
    want_t = (0.1, 10.0)
    rng = np.random.default_rng(7)
    for step in range(3):
        mn = rng.uniform(0.02, 1.5, 3).astype(np.float32)       # below and above the floor of 0.1 / 0.9
        minmax = np.stack([mn, mn + rng.uniform(1.0, 20.0, 3).astype(np.float32)], 1).astype(np.float32)
        ops.depth_bins_update(_cuda(minmax), tracker, 0.1, enc.depth_bins, binning)
        want_t, want_bins = S.bins_update(minmax, want_t, 0.1, D, binning)
        got_t = tracker.cpu().numpy()
        assert got_t.tobytes() == np.array(want_t, np.float64).tobytes(), (step, got_t, want_t)
        got_bins = enc.depth_bins.cpu().numpy()
        _same_bits(got_bins, want_bins, f"bins step {step}")
        _same_bits(got_bins, matching.depth_bins(want_t[0], want_t[1], D, binning).numpy(), f"depth_bins step {step}")
    assert enc.depth_bins.data_ptr() == storage and enc.depth_bins.shape == (D,)
    if D > 1:
        assert (np.diff(got_bins) > 0).all()

    # the next plane sweep reads exactly these bins: its lowest map is 1 / bins[argmin]
    B, C, h, w = 1, 8, 6, 8
    g = torch.Generator().manual_seed(3)
    cur = torch.rand(B, C, h, w, generator=g).cuda()
    look = torch.rand(B, 1, C, h, w, generator=g).cuda()
    K = torch.tensor([[[0.6 * w, 0, 0.5 * w, 0], [0, 0.9 * h, 0.5 * h, 0], [0, 0, 1, 0], [0, 0, 0, 1]]], dtype=torch.float32)
    T = torch.eye(4)[None, None].clone()
    T[0, 0, 0, 3] = 0.05
    _, _, argmin, lowest = ops.cost_volume(cur, look, T.cuda(), K.cuda(), torch.linalg.inv(K).cuda(), enc.depth_bins)
    want_low = (np.float32(1) / got_bins[argmin.cpu().numpy()]).astype(np.float32)
    _same_bits(lowest.cpu().numpy(), want_low, "lowest after the update")


def test_nan_minimum_keeps_the_floor():
    """Python's max(floor, nan) is floor: a NaN item leaves the tracker's minimum pulled to the floor and its maximum NaN."""
    from polardepth import ops
    minmax = np.array([[np.nan, np.nan], [0.5, 3.0]], np.float32)
    tracker = torch.tensor([0.2, 8.0], dtype=torch.float64, device="cuda")
    bins = torch.zeros(4, device="cuda")
    ops.depth_bins_update(_cuda(minmax), tracker, 0.1, bins, "linear")
    want_t, want_bins = S.bins_update(minmax, (0.2, 8.0), 0.1, 4, "linear")
    got = tracker.cpu().numpy()
    assert got[0] == want_t[0] == 0.2 * 0.99 + 0.1 * 0.01 and np.isnan(got[1]) and np.isnan(want_t[1])
    _same_bits(bins.cpu().numpy(), want_bins, "bins")


# ------------------------------------------------------------------ functional.student_loss, polardepth.student
TERM_TOL = 4 * 7.0e-06       # 4 x the largest relative error tests/test_step_reproj_oracle_gpu.py records for reproj_loss/s


def _loss_inputs(N=2, H=32, W=48):
    from polardepth._lib import lib, check, ptr, stream_ptr
    g = torch.Generator().manual_seed(5)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    img = lambda sx, sy: torch.stack([torch.stack([0.5 + 0.25 * torch.sin((xx + sx) / (2.1 + c) + 0.7 * c + n) *
                                                   torch.cos((yy + sy) / (2.9 - 0.4 * c)) for c in range(3)]) for n in range(N)])
    K = torch.eye(4).repeat(N, 1, 1)
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.65 * W, 0.9 * H, W / 2, H / 2
    poses = []
    for t in (0.04, -0.03):
        T = torch.eye(4).repeat(N, 1, 1)
        T[:, 0, 3] = t
        poses.append(T.cuda())
    disps = [(0.2 + 0.5 * torch.rand((N, 1, H >> s, W >> s), generator=g)).cuda().requires_grad_(True) for s in range(2)]
    depths = []
    for d in disps:
        out = torch.empty((N, 1, H, W), device="cuda")
        check(lib.pd_disp_to_depth(ptr(d.detach()), ptr(out), None, N, d.shape[2], d.shape[3], H, W, 0.1, 2.0, stream_ptr()),
              "pd_disp_to_depth")
        depths.append(out)
    monos = [(dp * (0.8 + 0.4 * torch.rand(dp.shape, generator=g).cuda())) for dp in depths]
    rmask = (torch.rand((N, H, W), generator=g) < 0.5).to(torch.uint8).cuda()
    valid = torch.tensor([[1.0, 1.0], [0.0, 1.0]]).cuda()
    return dict(disps=disps, depths=depths, monos=monos, rmask=rmask, valid=valid, K=K.cuda(), inv_K=torch.linalg.inv(K).cuda(),
                poses=poses, target=img(0, 0).cuda(), sources=[img(0.6, -0.3).cuda(), img(-0.5, 0.4).cuda()])


@pytest.mark.parametrize("avg", [False, True])
def test_student_loss_wires_the_chain_per_scale(avg):
    """functional.student_loss: per scale the pair equals ops.student_combine on the maps of the same ops chain bit for bit,
    equals an fp64 restatement from the warped frames it returns (trainer.py:1202-1236; bound: 4 x what the photometric step's
    oracle test records, 2.8e-5 relative), and its gradient reaches every disparity map; the teacher's depth gets none."""
    from oracle import reproj as OR
    from polardepth import functional as PF, ops
    d = _loss_inputs()
    cfg = PF.LossCfg([0, 1], 0.1, 2.0, 0.35, 1e-3, 32, 48)
    monos = [m.clone().requires_grad_(True) for m in d["monos"]]
    terms, sels, warped = PF.student_loss(cfg, d["disps"], d["depths"], monos, d["target"], d["sources"], d["K"], d["inv_K"],
                                          d["poses"], d["valid"], d["rmask"], avg=avg, details=True)
    assert len(terms) == len(sels) == len(warped) == 2
    valid = d["valid"].cpu() != 0
    r = (d["rmask"].cpu() != 0) & valid.any(1)[:, None, None]
    for s in range(2):
        with torch.no_grad():
            maps = [ops.reprojection_loss(ops.view_synthesis(d["depths"][s], src, d["K"], d["inv_K"], T)[0], d["target"])
                    for src, T in zip(d["sources"], d["poses"])]
            l0, l1, sel, _ = ops.student_combine(maps, d["rmask"], d["depths"][s], d["monos"][s], d["valid"], avg, details=True)
        assert torch.equal(l0, terms[s][0].detach()) and torch.equal(l1, terms[s][1].detach()) and torch.equal(sel, sels[s])
        m64 = [OR.reprojection_loss(wf.detach().double().cpu(), d["target"].double().cpu())[:, 0] for wf in warped[s]]
        if avg:
            cnt = valid.sum(1)[:, None, None].double()
            m = sum(torch.where(valid[:, f][:, None, None], m64[f], torch.zeros_like(m64[f])) for f in range(2)) / cnt
        else:
            big = torch.full_like(m64[0], float("inf"))
            m = torch.stack([torch.where(valid[:, f][:, None, None], m64[f], big) for f in range(2)], 1).min(1)[0]
        rd = r.double()
        want0 = (torch.where(r, m, torch.zeros_like(m)) * rd).sum() / (rd.sum() + 1e-7)
        want1 = ((d["depths"][s].double().cpu() - d["monos"][s].double().cpu())[:, 0].abs() * (1 - rd)).mean()
        for name, got, ref in (("reproj", terms[s][0].item(), want0.item()), ("consistency", terms[s][1].item(), want1.item())):
            err = abs(got - ref) / abs(ref)
            print(f"student_loss avg={avg} scale {s} {name}: dev {got:.8f} fp64 {ref:.10f} rel err {err:.2e} tol {TERM_TOL:.1e}")
            assert err <= TERM_TOL, (s, name, got, ref)
    total = sum(a + b for a, b in terms)
    total.backward()
    for s, disp in enumerate(d["disps"]):
        assert disp.grad is not None and torch.isfinite(disp.grad).all() and disp.grad.abs().max().item() > 0, s
    assert all(m.grad is None for m in monos)


def test_matching_augmentation_on_the_device():
    import random
    from polardepth.student import matching_augmentation
    g = torch.Generator().manual_seed(9)
    look = torch.rand((4, 2, 3, 8, 12), generator=g).cuda()
    poses = (torch.eye(4) + 0.1 * torch.rand((4, 2, 4, 4), generator=g)).cuda()
    color0 = torch.rand((4, 3, 8, 12), generator=g).cuda()
    seed = next(s for s in range(10000) if sorted(_codes(random.Random(s), 4)) == [0, 0, 1, 2])
    rng = random.Random(seed)
    codes = _codes(random.Random(seed), 4)
    aug, look2, poses2 = matching_augmentation(look, poses, color0, True, True, rng=rng)
    assert rng.random() == _after(seed, 4)                       # one draw per item, in batch order
    assert aug.tolist() == [float(c != 0) for c in codes]
    for b, c in enumerate(codes):
        want_look = color0[b][None].expand(2, -1, -1, -1) if c == 1 else look[b]
        assert torch.equal(look2[b], want_look), (b, c)
        assert torch.equal(poses2[b], torch.zeros_like(poses[b]) if c == 2 else poses[b]), (b, c)
    for is_train, enabled in ((False, True), (True, False)):     # no draw is consumed, nothing changes
        rng = random.Random(seed)
        aug, look2, poses2 = matching_augmentation(look, poses, color0, is_train, enabled, rng=rng)
        assert rng.random() == random.Random(seed).random() and not aug.any() and look2 is look and poses2 is poses


def _codes(rng, n):
    return [1 if x < 0.25 else (2 if x < 0.5 else 0) for x in (rng.random() for _ in range(n))]


def _after(seed, n):
    import random
    rng = random.Random(seed)
    for _ in range(n):
        rng.random()
    return rng.random()


def test_depth_bin_tracker_drives_the_encoder_bins():
    """DepthBinTracker: the Python formula of update_adaptive_depth_bins on the device, into the encoder's own bins; values()
    and load() round-trip; the encoder's forward leaves the bins alone when it is given no range."""
    from manydepth.networks import ResnetEncoderMatching
    from polardepth import matching, ops
    from polardepth.student import DepthBinTracker
    enc = ResnetEncoderMatching(18, False, 32, 48, adaptive_bins=True, min_depth_bin=0.1, max_depth_bin=2.0).cuda()
    tracker = DepthBinTracker(0.1, 2.0, torch.device("cuda"))
    assert tracker.values() == (0.1, 2.0)
    mono = (0.3 + 1.5 * torch.rand((2, 1, 32, 48), generator=torch.Generator().manual_seed(2))).cuda()
    lowest = torch.ones((2, 8, 12), device="cuda")
    minmax = ops.student_masks(lowest, lowest, mono, want_maps=False)[3]
    tracker.update(minmax, enc)
    mn = mono.min(-1)[0].min(-1)[0].mean().cpu().item()           # trainer.py:650-664
    mx = mono.max(-1)[0].max(-1)[0].mean().cpu().item()
    want = (0.1 * 0.99 + max(0.1, mn * 0.9) * 0.01, 2.0 * 0.99 + mx * 1.1 * 0.01)
    assert tracker.values() == want
    bins = matching.depth_bins(want[0], want[1], 96, "linear")
    assert torch.equal(enc.depth_bins.cpu(), bins)
    g = torch.Generator().manual_seed(4)
    K = torch.tensor([[[0.6 * 12, 0, 6.0, 0], [0, 0.9 * 8, 4.0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]]).repeat(2, 1, 1)
    T = torch.eye(4).repeat(2, 1, 1, 1)
    T[:, 0, 0, 3] = 0.05
    with torch.no_grad():
        enc(torch.rand((2, 3, 32, 48), generator=g).cuda(), torch.rand((2, 1, 3, 32, 48), generator=g).cuda(), T.cuda(), K.cuda(),
            torch.linalg.inv(K).cuda())
    assert torch.equal(enc.depth_bins.cpu(), bins)                # no range given: the device-side bins stand
    other = DepthBinTracker(0.1, 2.0, torch.device("cuda"))
    other.load(0.25, 3.5, enc)
    assert other.values() == (0.25, 3.5) and torch.equal(enc.depth_bins.cpu(), matching.depth_bins(0.25, 3.5, 96, "linear"))
