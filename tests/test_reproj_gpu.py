"""csrc/reproj.hip on the device against tests/reproj_ref.py (fp64 NumPy) and fixture G12 (the reference's own pieces run on
the CPU in float32 and float64, tests/golden/make_golden_reproj.py).

Bounds.  coords: the kernel evaluates the projection in fp64 and rounds once, the reference value is an fp64 evaluation in
another summation order rounded once -- both fp64 errors are far below half an fp32 ulp, so the two roundings differ by at
most one ulp (double rounding).  warped, fed the kernel's own coords (identical cells): two weight roundings (1 - w), a weight
product, a value product and three additions on values and weights in [0, 1]: at most 7 * 2^-24 ~ 4.2e-7 plus the weight
roundings, bound 1e-6 * max(1, max|src|).  Against the fixture: multiples of the reference's own float32 deviation from its
float64 run, as recorded in the fixture (1x in the mean; 2x in the maximum, a noisy statistic over ~2000 pixels).

The backward kernels on their own, nothing excluded.  pd_view_synth_bwd at the kernel's own coords: per pixel
(4 + C) * 2^-24 * A + 2^-24 |ref|, roundings counted in _assert_depth_gradient, A the reference with |.| on every summand.
pd_depth_to_updisp_bwd: 4 * 2^-24 |ref| (four roundings).  The whole term's disparity gradient: the rule of
tests/loss_cases.py (4 x the deviation of the same chain with its SSIM stage in fp32) at the device's own sel, count,
coords and warped images."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

import reproj_ref as R
from reproj_cases import combine_cases as _combine_cases      # shared with tests/test_oracle_reproj.py

pytestmark = pytest.mark.gpu
H, W = 19, 37


@pytest.fixture(scope="module")
def g12():
    return dict(np.load(os.path.join(GOLDEN, "g12_reproj.npz")))


@pytest.fixture(scope="module")
def synth(g12):
    """pd_view_synth_fwd on both source frames of the fixture, once: (warped, coords) as NumPy, and the device inputs."""
    from polardepth import ops
    dev = {k: torch.from_numpy(g12[k]).cuda() for k in ("depth", "target", "src0", "src1", "K", "inv_K", "T0", "T1", "noise",
                                                       "gw0", "gw1")}
    out = {}
    for f in range(2):
        warped, coords = ops.view_synthesis(dev["depth"], dev[f"src{f}"], dev["K"], dev["inv_K"], dev[f"T{f}"])
        out[f] = (warped.cpu().numpy(), coords.cpu().numpy())
    return out, dev


def _ulp_diff(got, want32):
    return np.abs(got.astype(np.float64) - want32.astype(np.float64)) / np.spacing(np.abs(want32)).astype(np.float64)


@pytest.mark.parametrize("f", [0, 1])
def test_coords_are_the_fp32_rounding_of_the_fp64_projection(g12, synth, f):
    _, coords = synth[0][f]
    assert coords.dtype == np.float32 and coords.shape == (2, H, W, 2)
    want = R.view_synth(g12["depth"], g12[f"src{f}"], g12["K"], g12["inv_K"], g12[f"T{f}"])["coords"].astype(np.float32)
    d = _ulp_diff(coords, want)
    print(f"coords frame {f}: max ulp {d.max()}, share exact {(d == 0).mean():.4f}")
    assert d.max() <= 1.0
    if f == 1:                                           # stored unclamped: the large pose leaves the image on every side
        assert coords[..., 0].min() < -1 and coords[..., 0].max() > W and coords[..., 1].min() < -1 and coords[..., 1].max() > H


@pytest.mark.parametrize("f", [0, 1])
def test_warped_matches_the_definition_at_the_kernels_own_coords(g12, synth, f):
    warped, coords = synth[0][f]
    want = R.sample(g12[f"src{f}"], coords)["warped"]
    err = np.abs(warped - want).max()
    bound = 1e-6 * max(1.0, np.abs(g12[f"src{f}"]).max())
    print(f"warped frame {f}: max |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_warped_against_the_reference_run(g12, synth):
    dev = np.concatenate([np.abs(synth[0][f][0] - g12[f"warped{f}_f64"]).ravel() for f in range(2)])
    print(f"warped vs reference fp64: mean {dev.mean():.3e} (reference fp32 {g12['dev_warped_mean']:.3e}), "
          f"max {dev.max():.3e} (reference fp32 {g12['dev_warped_max']:.3e})")
    assert dev.mean() <= 1.0 * g12["dev_warped_mean"]
    assert dev.max() <= 2.0 * g12["dev_warped_max"]


@pytest.mark.parametrize("f", [0, 1])
def test_depth_gradient_against_the_reference_autograd(g12, synth, f):
    from polardepth import ops
    dev = synth[1]
    depth = dev["depth"].clone().requires_grad_(True)
    warped, coords = ops.view_synthesis(depth, dev[f"src{f}"], dev["K"], dev["inv_K"], dev[f"T{f}"])
    assert not coords.requires_grad
    warped.backward(dev[f"gw{f}"])
    g = depth.grad.cpu().numpy().astype(np.float64)
    c = coords.cpu().numpy()
    near = R.near_boundary(c, H, W)[:, None]
    assert near.mean() <= 0.03, near.mean()
    want = g12[f"gdepth{f}_f64"]
    rel = np.abs(g - want)[~near].max() / np.abs(want).max()
    print(f"gdepth frame {f}: rel dev {rel:.3e} (reference fp32 {g12['dev_gdepth_rel']:.3e}), excluded {near.mean():.4f}")
    assert rel <= 2.0 * g12["dev_gdepth_rel"]
    s = R.sample(g12[f"src{f}"], c)
    both = ~s["free_x"] & ~s["free_y"]
    assert (g[:, 0][both] == 0).all()
    # one clamped axis contributes exactly nothing: the gradient is the other axis' alone
    one = R.view_synth_grad(g12[f"gw{f}"], g12[f"src{f}"], c, g12["depth"], g12["K"], g12["inv_K"], g12[f"T{f}"])
    only_y = (~s["free_x"] & s["free_y"] & ~near[:, 0])
    if f == 1:
        assert only_y.sum() > 50
    assert np.abs(g[:, 0][only_y] - one[:, 0][only_y]).max(initial=0.0) <= 2.0 * g12["dev_gdepth_rel"] * np.abs(want).max()


def test_backward_accumulate_flag_adds_to_what_is_there(g12, synth):
    from polardepth._lib import lib, check, ptr, stream_ptr
    dev = synth[1]
    coords = torch.from_numpy(synth[0][1][1]).cuda()
    args = lambda out, acc: (ptr(dev["gw1"]), ptr(dev["src1"]), ptr(coords), ptr(dev["depth"]), ptr(dev["K"]), ptr(dev["inv_K"]),
                             ptr(dev["T1"]), ptr(out), 2, 3, H, W, acc, stream_ptr())
    g = torch.empty_like(dev["depth"])
    check(lib.pd_view_synth_bwd(*args(g, 0)), "pd_view_synth_bwd")
    base = torch.full_like(g, 0.25)
    acc = base.clone()
    check(lib.pd_view_synth_bwd(*args(acc, 1)), "pd_view_synth_bwd")
    assert torch.equal(acc, base + g) and g.abs().max().item() > 0


def test_view_synthesis_grid_stride_and_non_finite_coordinates():
    """4 x 1 x 512 x 520: more pixels per item than one sweep of the per-item grid, so every workgroup strides; two columns
    of non-finite depth give non-finite coordinates, which sample source pixel 0 of both axes."""
    from polardepth import ops
    N, C, h, w = 4, 1, 512, 520
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float32)
    depth = np.stack([1.0 + 0.3 * np.sin(xx / 50.0 + n) * np.cos(yy / 40.0) for n in range(N)])[:, None].astype(np.float32)
    src = rng.random((N, C, h, w), dtype=np.float32)
    K = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    K[:, 0, 0] = K[:, 1, 1] = 0.6 * w
    K[:, 0, 2], K[:, 1, 2] = w / 2, h / 2
    inv_K = np.linalg.inv(K).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    T[:, 0, 3], T[:, 2, 3] = 0.03, -0.02
    depth[0, 0, :, 7] = np.nan                           # NaN and infinite depths: (u, v) = NaN (inf / inf)
    depth[0, 0, :, 9] = np.inf
    t = lambda a: torch.from_numpy(a).cuda()
    warped, coords = ops.view_synthesis(t(depth), t(src), t(K), t(inv_K), t(T))
    warped, coords = warped.cpu().numpy(), coords.cpu().numpy()
    assert not np.isfinite(coords[0, :, [7, 9]]).any() and np.isfinite(coords[1:]).all()
    assert np.array_equal(warped[0, 0, :, 7], np.full(h, src[0, 0, 0, 0])) and np.array_equal(warped[0, 0, :, 9], warped[0, 0, :, 7])
    fin = np.isfinite(coords)
    with np.errstate(all="ignore"):
        want = R.view_synth(depth, src, K, inv_K, T)["coords"]
    assert _ulp_diff(coords[fin], want[fin].astype(np.float32)).max() <= 1.0
    assert np.abs(warped - R.sample(src, coords)["warped"]).max() <= 1e-6


# ------------------------------------------------------------------ the reduction over the frames
def _run_combine(reproj, identity=None, noise=None, valid=None, avg=False):
    from polardepth import ops
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    maps = [t(r).requires_grad_(True) for r in reproj]
    loss, sel, sums = ops.reproj_combine(maps, None if identity is None else [t(i) for i in identity], t(noise), t(valid), avg,
                                         details=True)
    loss.backward(torch.tensor(1.5, device="cuda"))
    return loss.detach().cpu().numpy(), sel.cpu().numpy(), sums.cpu().numpy(), [m.grad.cpu().numpy() for m in maps]


@pytest.mark.parametrize("case", ["fixture", "no_noise", "no_automask", "avg", "avg_invalid", "item_without_frames",
                                  "first_frame_invalid", "tie_between_frames", "tie_with_identity"])
def test_combine_selection_count_and_sums(g12, case):
    kw = _combine_cases(g12)[case]
    want = R.combine(**kw)
    loss, sel, sums, grads = _run_combine(**kw)
    loss2, sel2, sums2, grads2 = _run_combine(**kw)
    assert np.array_equal(sel, want["sel"]), (sel != want["sel"]).sum()
    assert sums[1] == want["count"]
    n = sel.size
    print(f"{case}: sum {sums[0]!r} vs {want['sum']!r}, count {sums[1]}, loss {loss}")
    assert abs(sums[0] - want["sum"]) <= n * 2.0 ** -52 * want["abs_sum"]
    assert loss == np.float32(sums[0] / (sums[1] + 1e-7))
    assert loss.tobytes() == loss2.tobytes() and sums.tobytes() == sums2.tobytes() and np.array_equal(sel, sel2)
    assert all(np.array_equal(a, b) for a, b in zip(grads, grads2))
    # backward: gloss / (count + 1e-7) rounded once (avg: one more division by the number of valid frames), 3 ulp
    for g, w in zip(grads, R.combine_grad(1.5, want["sel"], want["count"], kw.get("valid"), 2, kw.get("avg", False))):
        assert np.array_equal(g != 0, w != 0)
        assert np.abs(g - w).max() <= 3 * 2.0 ** -24 * np.abs(w).max() + 0.0
    if case == "item_without_frames":
        assert (sel[0] == 255).all() and (sel[1] != 255).any() and all((g[0] == 0).all() for g in grads)
    if case == "tie_between_frames":
        assert (sel[:, 3:9] == 0).all() and (sel == 1).any()
    if case == "tie_with_identity":
        assert (sel[0, :5] != 255).all()
    if case == "no_automask":
        assert sums[1] == n and (sel != 255).all()
    if case == "first_frame_invalid":
        assert set(np.unique(sel[0])) <= {1, 255} and set(np.unique(sel[1])) <= {0, 255}


def test_combine_grid_stride_is_reproducible_and_exact_in_count():
    """3 x 512 x 384 pixels: more than the 2048 workgroups of 256 threads cover in one sweep."""
    from polardepth import ops
    gen = torch.Generator(device="cuda").manual_seed(4)
    shape = (3, 1, 512, 384)
    r = [torch.rand(shape, generator=gen, device="cuda") for _ in range(3)]
    i = [torch.rand(shape, generator=gen, device="cuda") for _ in range(3)]
    out = [ops.reproj_combine(r, i, details=True) for _ in range(2)]
    m = torch.minimum(torch.minimum(r[0], r[1]), r[2])
    keep = m <= torch.minimum(torch.minimum(i[0], i[1]), i[2])
    total = (m.double() * keep).sum().item()
    loss, sel, sums = out[0]
    assert sums[1].item() == keep.sum().item() and torch.equal((sel != 255)[:, None], keep)
    assert abs(sums[0].item() - total) <= keep.numel() * 2.0 ** -52 * total
    assert torch.equal(sel, out[1][1]) and torch.equal(sums, out[1][2]) and torch.equal(loss, out[1][0])
    assert torch.equal(sel[keep[:, 0]].long(), torch.stack(r, 0).argmin(0)[keep])


# ------------------------------------------------------------------ the whole term
def _cfg():
    from polardepth import functional as PF
    return PF.LossCfg([0], 0.1, 2.0, 0.35, 1e-3, H, W)


def test_photometric_loss_end_to_end_with_the_stored_noise(g12, synth):
    from polardepth import functional as PF
    dev = synth[1]
    valid = torch.ones(2, 2, device="cuda")
    losses, sels = PF.photometric_loss(_cfg(), None, [dev["depth"]], dev["target"], [dev["src0"], dev["src1"]], dev["K"],
                                       dev["inv_K"], [dev["T0"], dev["T1"]], valid, noise=dev["noise"], details=True)
    assert len(losses) == 1 and losses[0].shape == ()
    near = g12["near_tie"][:, 0]
    assert near.mean() <= 0.01
    want_sel = np.where(g12["mask_f64"][:, 0] != 0, g12["argmin_f64"][:, 0], 255).astype(np.uint8)
    sel = sels[0].cpu().numpy()
    print(f"selection: {(sel != want_sel)[~near].sum()} of {sel.size} differ; near ties {near.mean():.4f}")
    assert np.array_equal(sel[~near], want_sel[~near])
    err = abs(losses[0].item() - float(g12["loss_f64"]))
    bound = max(2.0 * float(g12["dev_loss"]), 1e-6)
    print(f"loss {losses[0].item()!r} vs {float(g12['loss_f64'])!r}: |err| {err:.3e} (bound {bound:.3e})")
    assert err <= bound


def test_photometric_loss_options_and_the_link_to_the_disparities():
    """--no_ssim, --disable_automasking and --avg_reprojection change the term; through DispDepthFn every scale's disparity
    receives a gradient, and that link equals torch's autograd of 1 / (min_disp + (max_disp - min_disp) * up(disp))."""
    from polardepth import functional as PF, synthetic
    from polardepth._lib import lib, check, ptr, stream_ptr
    b = synthetic.multiview_plane(2, 32, 48, seed=1)
    cfg = PF.LossCfg([0, 1], 0.1, 2.0, 0.35, 1e-3, 32, 48)
    gen = torch.Generator(device="cuda").manual_seed(0)
    disps = [(0.3 + 0.4 * torch.rand((2, 1, 32 >> s, 48 >> s), generator=gen, device="cuda")).requires_grad_(True) for s in (0, 1)]
    depths = []
    for d in disps:
        out = torch.empty((2, 1, 32, 48), device="cuda")
        check(lib.pd_disp_to_depth(ptr(d.detach()), ptr(out), None, 2, d.shape[2], d.shape[3], 32, 48, 0.1, 2.0, stream_ptr()),
              "pd_disp_to_depth")
        depths.append(out)
    args = (b[("color", 0, 0)], [b[("color", -1, 0)], b[("color", 1, 0)]], b[("K", 0)], b[("inv_K", 0)],
            [b[("poses", -1)], b[("poses", 1)]], torch.ones(2, 2, device="cuda"))
    base = PF.photometric_loss(cfg, disps, depths, *args)
    assert len(base) == 2 and all(torch.isfinite(l) for l in base)
    (base[0] + base[1]).backward()
    assert all(d.grad is not None and torch.isfinite(d.grad).all() and d.grad.abs().max().item() > 0 for d in disps)
    with torch.no_grad():
        variants = {k: float(PF.photometric_loss(cfg, None, depths, *args, **kw)[0]) for k, kw in
                    (("base", {}), ("no_ssim", {"no_ssim": True}), ("no_automask", {"automask": False}), ("avg", {"avg": True}))}
    assert base[0].item() == variants["base"] and len(set(variants.values())) == 4, variants
    # the link alone, against torch (fp32 on both sides: a few ulp of the largest entry)
    d1 = disps[1].detach().clone().requires_grad_(True)
    g = torch.randn((2, 1, 32, 48), generator=gen, device="cuda")
    PF.DispDepthFn.apply(d1, depths[1], 0.1, 2.0).backward(g)
    d2 = disps[1].detach().clone().requires_grad_(True)
    up = torch.nn.functional.interpolate(d2, [32, 48], mode="bilinear", align_corners=False)
    ref = 1.0 / (1 / 2.0 + (1 / 0.1 - 1 / 2.0) * up)
    assert (ref - depths[1]).abs().max().item() <= 1e-5
    ref.backward(g)
    assert (d1.grad - d2.grad).abs().max().item() <= 1e-5 * d2.grad.abs().max().item()


def test_conventions_true_depth_beats_scaled_depths_on_the_plane():
    from polardepth import functional as PF, synthetic
    b = synthetic.multiview_plane(2, 32, 48, frame_ids=(0, -1, 1), seed=0)
    cfg = PF.LossCfg([0], 0.1, 2.0, 0.35, 1e-3, 32, 48)
    vals = {}
    for s in (0.9, 1.0, 1.1):
        vals[s] = float(PF.photometric_loss(cfg, None, [b["depth"] * s], b[("color", 0, 0)],
                                            [b[("color", -1, 0)], b[("color", 1, 0)]], b[("K", 0)], b[("inv_K", 0)],
                                            [b[("poses", -1)], b[("poses", 1)]],
                                            torch.stack([b[("frame_valid", -1)], b[("frame_valid", 1)]], 1))[0])
    print("plane:", vals)
    assert vals[1.0] < vals[0.9] and vals[1.0] < vals[1.1]


# ------------------------------------------------------------------ the backward kernels, pixel by pixel
def _view_synth_bwd(gw, src, coords, depth, K, inv_K, T):
    from polardepth._lib import lib, check, ptr, stream_ptr
    N, C, h, w = src.shape
    g = torch.full((N, 1, h, w), float("nan"), device="cuda")
    check(lib.pd_view_synth_bwd(ptr(gw), ptr(src), ptr(coords), ptr(depth), ptr(K), ptr(inv_K), ptr(T), ptr(g), N, C, h, w, 0,
                                stream_ptr()), "pd_view_synth_bwd")
    torch.cuda.synchronize()
    return g.cpu().numpy().astype(np.float64)


def _assert_depth_gradient(g, gw, src, coords, depth, K, inv_K, T, what):
    """|g - ref| <= k 2^-24 A + 2^-24 |ref| on EVERY pixel, A = the reference expression with the absolute value of every
    summand (reproj_ref.view_synth_grad(magnitude=True)).  k = 4 + C, the fp32 roundings on the longest path to gu (or gv):
    the lower weight 1 - w1 (1), a tap difference (1), its product with the weight (1), the sum of the two products (1),
    the product with gw_c (1) -- 5 for a channel term -- and C - 1 additions of channel terms (the first lands on 0).  The
    rest (projection, du, dv, gu du + gv dv) is fp64 and rounded once: 2^-24 |ref|."""
    C = src.shape[1]
    a = (gw, src, coords, depth, K, inv_K, T)
    ref = R.view_synth_grad(*a)
    mag = R.view_synth_grad(*a, magnitude=True)
    bound = (4 + C) * 2.0 ** -24 * mag + 2.0 ** -24 * np.abs(ref)
    err = np.abs(g - ref)
    worst = np.argmax(err - bound)
    print(f"{what}: max err {err.max():.3e}, largest err / bound {(err / np.maximum(bound, 1e-300)).max():.3f}, "
          f"k = {4 + C}, every one of {err.size} pixels compared")
    assert (err <= bound).all(), (what, err.ravel()[worst], bound.ravel()[worst])
    s = R.sample(src, coords)
    both = ~s["free_x"] & ~s["free_y"]
    one = s["free_x"] ^ s["free_y"]
    assert (g[:, 0][both] == 0).all()
    return one, both, s


@pytest.mark.parametrize("f", [0, 1])
def test_depth_gradient_at_the_kernels_own_coords_on_every_pixel(g12, synth, f):
    dev = synth[1]
    coords = synth[0][f][1]
    g = _view_synth_bwd(dev[f"gw{f}"], dev[f"src{f}"], torch.from_numpy(coords).cuda(), dev["depth"], dev["K"], dev["inv_K"],
                        dev[f"T{f}"])
    one, both, s = _assert_depth_gradient(g, g12[f"gw{f}"], g12[f"src{f}"], coords, g12["depth"], g12["K"], g12["inv_K"],
                                          g12[f"T{f}"], f"gdepth frame {f}")
    print(f"frame {f}: {one.sum()} pixels with one clamped axis, {both.sum()} with both")
    if f == 1:                                           # leaves the image on every side
        assert one.sum() >= 50 and both.sum() >= 50
        assert (~s["free_x"] & s["free_y"]).any() and (s["free_x"] & ~s["free_y"]).any()
        assert (g[:, 0][one] != 0).mean() > 0.9          # the single-axis value (inside the bound above), not a zero


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (1, 2, 3, 5)])
def test_depth_gradient_on_tiny_images_where_the_upper_tap_clamps_at_the_last_cell(shape):
    """Identity plus a small translation: the last column's coordinate passes W - 1, its cell is i0 = i1 = W - 1."""
    from polardepth import ops
    N, C, h, w = shape
    rng = np.random.default_rng(h * w)
    depth = (1.0 + 0.2 * rng.random((N, 1, h, w))).astype(np.float32)
    src = rng.random(shape, dtype=np.float32)
    gw = rng.standard_normal(shape).astype(np.float32)
    K = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    K[:, 0, 0], K[:, 1, 1], K[:, 0, 2], K[:, 1, 2] = 0.9 * w, 1.1 * h, (w - 1) / 2 + 0.1, (h - 1) / 2 - 0.1
    inv_K = np.linalg.inv(K).astype(np.float32)
    T = np.tile(np.eye(4, dtype=np.float32), (N, 1, 1))
    T[:, 0, 3], T[:, 1, 3], T[:, 2, 3] = 0.08, -0.03, 0.02
    t = lambda a: torch.from_numpy(a).cuda()
    warped, coords = ops.view_synthesis(t(depth), t(src), t(K), t(inv_K), t(T))
    c = coords.cpu().numpy()
    assert (c[..., 0] >= w - 1).any() and ((c[..., 0] > 0) & (c[..., 0] < w - 1)).any()
    assert np.abs(warped.cpu().numpy() - R.sample(src, c)["warped"]).max() <= 1e-6
    g = _view_synth_bwd(t(gw), t(src), coords, t(depth), t(K), t(inv_K), t(T))
    one, both, _ = _assert_depth_gradient(g, gw, src, c, depth, K, inv_K, T, f"gdepth {shape}")
    assert one.any() or both.any()


@pytest.mark.parametrize("n", [1, 255, 257, 2048 * 256 + 3])
def test_depth_to_updisp_backward_elementwise(n):
    """gup = -g d^2 (1 / min - 1 / max) in fp64, per element within 4 * 2^-24 |ref|: the range, d d, its product with the range
    and the product with g.  (With min = 0.1, max = 2 the range 1.f / 0.1f - 1.f / 2.f is 9.5 exactly.)  The last size
    takes the grid-stride loop past its first trip; zero and mirrored gradients give exact zeros and exact symmetry."""
    from polardepth._lib import lib, check, ptr, stream_ptr
    gen = torch.Generator().manual_seed(n)
    d = (0.1 + 1.9 * torch.rand(n, generator=gen)).float()
    d[0], d[-1] = 0.1, 2.0                                # spans [min_depth, max_depth] (n == 1: max_depth)
    g = torch.randn(n, generator=gen)
    g[::5] = 0.0
    run = lambda gg: _updisp_bwd(lib, check, ptr, stream_ptr, gg, d)
    got, neg = run(g), run(-g)
    ref = -g.double() * d.double() ** 2 * (1 / 0.1 - 1 / 2.0)
    err = (got.double() - ref).abs()
    print(f"updisp bwd n = {n}: max err / |ref| {(err / ref.abs().clamp_min(1e-300)).max().item() / 2.0 ** -24:.3f} x 2^-24")
    assert (err <= 4 * 2.0 ** -24 * ref.abs()).all()
    assert (got[::5] == 0).all() and torch.equal(neg, -got)
    assert n == 1 or (got[1::5] != 0).all()


def _updisp_bwd(lib, check, ptr, stream_ptr, g, d):
    n = g.numel()
    out = torch.full((n + 64,), -7.25, device="cuda")
    gd, dd = g.cuda(), d.cuda()                           # named: a temporary's block would be handed to the next one
    check(lib.pd_depth_to_updisp_bwd(ptr(gd), ptr(dd), ptr(out), n, 0.1, 2.0, stream_ptr()), "pd_depth_to_updisp_bwd")
    torch.cuda.synchronize()
    assert (out[n:] == -7.25).all()
    return out[:n].cpu()


# ------------------------------------------------------------------ the whole term's disparity gradient
def test_photometric_term_disparity_gradient_against_the_fp64_chain(g12, synth):
    """d (loss_0 + loss_1) / d disparity of PF.photometric_loss at two scales against the chain of the
    pieces in fp64, evaluated at the device's own discrete intermediates (sel, count, coords, warped):
        reproj_ref.combine_grad -> autograd of the fp64 photometric mix at (warped, target) -> reproj_ref.view_synth_grad,
        summed over the frames -> -g d^2 range -> loss_cases.ref_gather.
    The yardstick is the same chain with the mix in fp32; the rule of loss_cases elementwise.  Excluded: disparity pixels
    whose footprint touches an SSIM gate-undecided pixel of the winning frame -- none on the fixture's images (asserted,
    cap 5 %; tests/test_reproj_ref.py shows the same on the fp64 images), so no blending toward the target (factor 0).
    The scales are 19 x 37 and 1 x 37: pd_up_gather_bwd takes integer zoom factors only and 19 and 37 are prime, so the
    coarser map of this fixture can only drop a whole axis (zoom 19 x 1, the any-ratio gather kernel)."""
    import loss_cases as lc
    import ssim_cases as sc
    from polardepth import functional as PF, ops
    from polardepth._lib import lib, check, ptr, stream_ptr
    dev = synth[1]
    N = 2
    sizes = [(H, W), (1, W)]
    rng_d = 1 / 0.1 - 1 / 2.0
    fix = dev["depth"]
    disps, depths = [], []
    for hs, ws in sizes:
        dsmall = fix if (hs, ws) == (H, W) else torch.nn.functional.interpolate(fix, size=(hs, ws), mode="bilinear", align_corners=False)
        disp = ((1.0 / dsmall - 1 / 2.0) / rng_d).contiguous()
        out = torch.empty((N, 1, H, W), device="cuda")
        check(lib.pd_disp_to_depth(ptr(disp), ptr(out), None, N, hs, ws, H, W, 0.1, 2.0, stream_ptr()), "pd_disp_to_depth")
        assert out.min().item() >= g12["depth"].min() - 1e-3 and out.max().item() <= g12["depth"].max() + 1e-3
        disps.append(disp.requires_grad_(True))
        depths.append(out)
    cfg = PF.LossCfg([0, 1], 0.1, 2.0, 0.35, 1e-3, H, W)
    srcs, poses = [dev["src0"], dev["src1"]], [dev["T0"], dev["T1"]]
    valid = torch.ones(N, 2, device="cuda")
    losses, sels = PF.photometric_loss(cfg, disps, depths, dev["target"], srcs, dev["K"], dev["inv_K"], poses, valid,
                                       noise=dev["noise"], details=True)
    (losses[0] + losses[1]).backward()
    with torch.no_grad():
        identity = [ops.reprojection_loss(s, dev["target"]) for s in srcs]
    tgt = torch.from_numpy(g12["target"])
    for i, (hs, ws) in enumerate(sizes):
        synth_i = [ops.view_synthesis(depths[i], s, dev["K"], dev["inv_K"], T) for s, T in zip(srcs, poses)]
        again = [ops.view_synthesis(depths[i], s, dev["K"], dev["inv_K"], T) for s, T in zip(srcs, poses)]
        assert all(torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) for a, b in zip(synth_i, again))
        maps = [ops.reprojection_loss(w, dev["target"]) for w, _ in synth_i]
        loss, sel, sums = ops.reproj_combine(maps, identity, dev["noise"], valid, False, details=True)
        # the separate calls reproduce what the term computed inside, bit for bit
        assert torch.equal(loss, losses[i].detach()) and torch.equal(sel, sels[i])
        sel_np, count = sel.cpu().numpy(), float(sums[1].item())
        assert 0 < count < sel_np.size and (sel_np == 0).any() and (sel_np == 1).any()
        gmaps = R.combine_grad(1.0, sel_np, count, None, 2)
        depth_np = depths[i].cpu().numpy()
        und = torch.zeros(N, 1, H, W, dtype=torch.bool)
        chain = {}
        for dt in (sc.F32, sc.F64):
            gdepth = np.zeros((N, 1, H, W))
            for f in range(2):
                warped = synth_i[f][0].cpu()
                gw = sc.ref_grads(warped, tgt, torch.from_numpy(gmaps[f]), dt, 1)[0].double().numpy()
                gdepth += R.view_synth_grad(gw, g12[f"src{f}"], synth_i[f][1].cpu().numpy(), depth_np, g12["K"], g12["inv_K"],
                                            g12[f"T{f}"])
                if dt == sc.F64:
                    u = sc.gate_undecided(warped, tgt).any(1, keepdim=True) & torch.from_numpy(sel_np == f)[:, None]
                    und |= torch.nn.functional.max_pool2d(u.double(), 5, 1, 2) > 0
            gup = torch.from_numpy(-gdepth * depth_np.astype(np.float64) ** 2 * rng_d)
            chain[dt] = lc.ref_gather(gup, hs, ws, torch.float64)
        keep = lc.ref_gather(und.double(), hs, ws, torch.float64) == 0
        excluded = 1.0 - keep.double().mean().item()
        assert excluded <= 0.05
        got = disps[i].grad.cpu()
        assert got.abs().max().item() > 0
        err, tol = lc.assert_elem(got[keep], chain[sc.F32][keep], chain[sc.F64][keep], f"disparity gradient scale {i}")
        print(f"REPROJFIG | disparity gradient {hs} x {ws} | err {err:.2e} | tol {tol:.2e} | excluded {excluded:.4f} | "
              f"scale of the gradient {chain[sc.F64].abs().max().item():.2e}")
