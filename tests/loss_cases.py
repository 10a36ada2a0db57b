"""Shared by tests/test_loss_cases.py (CPU) and tests/test_loss_kernels_gpu.py (GPU): the named geometries and inputs of
the K5 loss kernels (csrc/loss.hip), with the edge populations written in (ties, holes, exact mask bounds, a wholly masked
image), the fp64 references, and the comparison rule as code.

References are the functions of oracle/losses.py evaluated in the requested dtype (fp32 = the yardstick, fp64 = the truth).
The few restatements below (edge-weight map, per-image mean, bookkeeping arithmetic) follow the reference formulas quoted
in the header comment of csrc/loss.hip (trainer.py:1241-1265, layers.py:452-465), not the kernels.

Comparison rule (nothing fitted to a device result):
  elementwise   |dev - ref64| <= 4 * max|ref32 - ref64| + 1e-6 * max|ref64|
  scalar sums   |dev - ref64| <= 4 * |ref32 - ref64| + 1e-6 * |ref64|
  counts        exact
The kernels are fp32 evaluations of the same formulas in another summation order, with fused reciprocals: the precision
class of the fp32 oracle, hence a small multiple (4) of its own deviation from fp64."""
import math

import torch
import torch.nn.functional as F

from oracle import losses as ol

MIN_D, MAX_D = 0.1, 2.0
LO = float(torch.tensor(MIN_D, dtype=torch.float32))      # float32(0.1), the value the kernels compare with
HI = float(torch.tensor(MAX_D, dtype=torch.float32))
DISP_RANGE = 1.0 / MIN_D - 1.0 / MAX_D
GRID_CAP = 2048 * 256                                     # pixels one K5 launch covers without a second grid-stride trip
TILE_CAP = 4096                                           # tiles of the fused backward kernel per trip
TILE_R, TILE_C = 8, 64
COND = 1e-5                                               # cap on |oracle32 - oracle64| / scale, every case, every pixel

SUP_GEOMS = [(2, 21, 70), (1, 8, 130), (3, 1, 40), (2, 40, 1), (1, 2, 2), (1, 32808, 17)]
SUP_BWD_GEOMS = SUP_GEOMS + [(2, 9, 65), (1, 17, 129)]
SUP_WTS = (0.7, 0.455, 1e-3)                              # non-uniform (w_L1, w_LN, w_sm)


# ====================================================================================================== comparison rule
def elem_tol(ref32, ref64):
    ref64 = ref64.double()
    return 4.0 * (ref32.double() - ref64).abs().max().item() + 1e-6 * ref64.abs().max().item()


def assert_elem(dev, ref32, ref64, what):
    """Every element within the rule; returns (worst error, tolerance) for the tables."""
    dev = torch.as_tensor(dev).detach().cpu().double()
    ref64 = ref64.detach().double()
    assert dev.shape == ref64.shape, f"{what}: shape {tuple(dev.shape)} vs {tuple(ref64.shape)}"
    assert torch.isfinite(dev).all(), f"{what}: non-finite device output"
    tol = elem_tol(ref32.detach(), ref64)
    err = (dev - ref64).abs().max().item() if dev.numel() else 0.0
    assert err <= tol, f"{what}: max err {err:.3e} > tol {tol:.3e} (scale {ref64.abs().max().item():.3e})"
    return err, tol


def assert_scalar(dev, ref32, ref64, what):
    dev, ref32, ref64 = float(torch.as_tensor(dev).detach()), float(ref32), float(ref64)
    tol = 4.0 * abs(ref32 - ref64) + 1e-6 * abs(ref64)
    assert math.isfinite(dev) and abs(dev - ref64) <= tol, f"{what}: {dev!r} vs {ref64!r}, tol {tol:.3e}"
    return abs(dev - ref64), tol


def conditioning(ref32, ref64):
    """max |oracle32 - oracle64| / max |oracle64| (0 for an all-zero reference)."""
    s = ref64.double().abs().max().item()
    return 0.0 if s == 0.0 else (ref32.double() - ref64.double()).abs().max().item() / s


# ====================================================================================================== supervised terms
def make_K(N, H, W):
    """Distinct per image, principal point off centre, fx != fy."""
    K = torch.eye(4)[None].repeat(N, 1, 1)
    for n in range(N):
        K[n, 0, 0] = 0.9 * W * (1 + 0.05 * n) + 0.3
        K[n, 1, 1] = 1.1 * H * (1 + 0.03 * n) + 0.2
        K[n, 0, 2] = 0.5 * W + 0.7 + 0.3 * n
        K[n, 1, 2] = 0.5 * H - 0.4 + 0.15 * n
    return K


def _grid(H, W):
    return torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")


def sup_case(N, H, W, dead_image=None):
    """gt, pred [N,1,H,W], K [N,4,4] and the populations written into them (boolean maps).

    gt: 1 + 0.5 sin(x/9) cos(y/7) + 0.02 U per image (H > 256: a sawtooth in y, and the populations below as whole rows),
        then by flat pixel index p of every image
        p % 11 == 3 -> 0 (hole), p % 13 == 5 -> 5.0 / 0.05 (out of range), p % 17 == 7 -> float32(0.1), p % 19 == 9 ->
        float32(2.0); a hole patch and an out-of-range patch where the image is large enough; images of fewer than 20
        pixels carry float32(0.1), float32(2.0) and a hole at p = 0, 1, 3.  dead_image: that image wholly out of range.
    pred: another smooth surface in (0.5, 1.6); equal to gt bit for bit on the in-range pixels of a block (ties)."""
    g = torch.Generator().manual_seed(1000 * N + 10 * H + W)
    yy, xx = _grid(H, W)
    if H > 256:
        # tall image: |y - cy| reaches 2^14, and the fp32 rounding of Y = (y - cy) / fy * d is 2^-24 |y - cy| of the term d / fy
        # that is left of dY/dy where the depth is flat in y.  A sawtooth in y (0.05 per row, then the drop, in the same row
        # of every column) keeps dY/dy dominated by (y - cy) dd/dy, whose relative rounding is 2^-24 d / |dd/dy| ~ 2e-6.
        # pred = that surface -+ 0.05 by column: whichever rows of it are replaced by gt (ties) or kept where gt is a hole,
        # the difference of two rows in a column is 0.05, 0.1 or 0.15 or the drop, never near zero.
        gt = torch.stack([0.7 + 0.9 * torch.frac(yy / 18.0 + 0.1 * n) + 0.1 * torch.sin(xx / 3.0) for n in range(N)])[:, None]
        pred = gt + torch.where(xx % 2 == 0, 0.05, -0.05)
        noise = 0.002
    else:
        gt = torch.stack([1.0 + 0.5 * torch.sin(xx / 9.0 + 0.4 * n) * torch.cos(yy / 7.0) for n in range(N)])[:, None]
        pred = torch.stack([1.05 + 0.4 * torch.sin(xx / 11.0 + 0.5) * torch.cos(yy / 8.0 + 0.3 * n) for n in range(N)])[:, None]
        noise = 0.02
    gt = gt + noise * torch.rand(N, 1, H, W, generator=g)
    pred = pred + noise * torch.rand(N, 1, H, W, generator=g)
    p = torch.arange(H * W).view(1, 1, H, W).expand(N, 1, H, W)
    if H * W < 20:
        gt.view(N, -1)[:, 0] = LO
        gt.view(N, -1)[:, 1] = HI
        gt.view(N, -1)[:, 3] = 0.0
    elif H > 256:
        # whole rows: single special pixels scattered over 5e5 pixels meet in Sobel windows whose y-sum cancels by chance
        row = torch.arange(H).view(1, 1, H, 1).expand(N, 1, H, W)
        gt[row % 97 == 3] = 0.0
        gt[row % 101 == 5] = 5.0
        gt[row % 211 == 6] = 0.05
        gt[row % 103 == 7] = LO
        gt[row % 107 == 9] = HI
    else:
        gt[p % 11 == 3] = 0.0
        gt[(p % 13 == 5) & (p % 2 == 0)] = 5.0
        gt[(p % 13 == 5) & (p % 2 == 1)] = 0.05
        gt[p % 17 == 7] = LO
        gt[p % 19 == 9] = HI
    if H > 6 and W > 12:
        gt[:, :, 1:4, 2:6] = 0.0
        gt[:, :, 3:6, 8:12] = 5.0
    if dead_image is not None:
        gt[dead_image] = 2.5 + 0.1 * torch.rand(1, H, W, generator=g)
    valid = (gt >= LO) & (gt <= HI)
    if H * W < 64:
        block = p % 3 == 2
    else:
        block = torch.zeros(N, 1, H, W, dtype=torch.bool)
        block[:, :, H // 3:max(2 * H // 3, H // 3 + 1), W // 3:max(2 * W // 3, W // 3 + 1)] = True
    tie = block & valid
    pred = torch.where(tie, gt, pred)
    return dict(N=N, H=H, W=W, gt=gt.contiguous(), pred=pred.contiguous(), K=make_K(N, H, W), valid=valid, tie=tie,
                at_lo=gt == LO, at_hi=gt == HI, hole=gt == 0.0)


def ref_gt_normals(c, dt):
    """[N,H,W,3]: ol.depth_to_normals of the ground truth, zero outside the depth-range mask."""
    gt, K = c["gt"].to(dt), c["K"].to(dt)
    m = ((gt >= LO) & (gt <= HI)).to(dt)
    return (ol.depth_to_normals(gt, K[:, :3, :3]) * m).permute(0, 2, 3, 1).contiguous()


def ref_sup_sums(c, dt, with_normals=True):
    """(sum |gt - d| m, sum (2 - cos) m, sum m): numerators and denominator of trainer.py:1241-1251 and 1298-1309."""
    gt, pred, K = c["gt"].to(dt), c["pred"].to(dt), c["K"].to(dt)
    m = ((gt >= LO) & (gt <= HI)).to(dt)
    cnt = m.sum()
    l1 = (torch.abs(gt - pred) * m).sum()
    ln = ol.normals_loss(gt, pred, K, m) * cnt if with_normals else torch.zeros((), dtype=dt)
    return l1, ln, cnt


def ref_sup_grad(c, dt, with_normals, to_disp, wts=SUP_WTS):
    """d (w0 L1 + w1 LN) / d pred by autograd.  to_disp: with respect to the upsampled disparity u, depth = 1 / (1/max +
    range u), by the chain rule d depth / d u = -range depth^2 on the same depth values: re-deriving the depth from u
    in floating point would move it off gt by an ulp on the tie pixels and replace sign(0) = 0 by +-1 in the reference."""
    gt, K = c["gt"].to(dt), c["K"].to(dt)
    pred = c["pred"].to(dt).clone().requires_grad_(True)
    m = ((gt >= LO) & (gt <= HI)).to(dt)
    w = torch.tensor(wts, dtype=torch.float32).to(dt)
    loss = w[0] * (torch.abs(gt - pred) * m).sum() / m.sum()
    if with_normals:
        loss = loss + w[1] * ol.normals_loss(gt, pred, K, m)
    loss.backward()
    g = pred.grad
    if to_disp:
        g = g * (-(1.0 / torch.tensor(LO, dtype=dt) - 1.0 / torch.tensor(HI, dtype=dt)) * pred.detach() ** 2)
    return g


def ref_normals_loss_masked(c, mask, dt):
    return ol.normals_loss(c["gt"].to(dt), c["pred"].to(dt), c["K"].to(dt), mask.to(dt))


def arbitrary_mask(c):
    """A weight map that is not the depth-range mask: 0 / 0.5 / 1 by pixel index, holes included."""
    N, H, W = c["N"], c["H"], c["W"]
    p = torch.arange(H * W).view(1, 1, H, W).expand(N, 1, H, W)
    return torch.where(p % 3 == 0, 0.0, torch.where(p % 2 == 0, 0.5, 1.0)).contiguous()


def late_tile_rows(N, H, W):
    """Rows (of image N-1) that lie in tiles with index >= TILE_CAP of the fused backward kernel, or None."""
    th, tw = -(-H // TILE_R), -(-W // TILE_C)
    if N * th * tw <= TILE_CAP:
        return None
    first = TILE_CAP - (N - 1) * th * tw                   # first late tile, within the last image
    assert first >= 0
    return (first // tw) * TILE_R + (TILE_R if first % tw else 0)       # rows whose tiles are all late


# ====================================================================================================== up / down sampling
# (N, hs, ws, H, W)
D2D_CASES = [(2, 6, 10, 6, 10), (2, 6, 10, 12, 20), (2, 6, 10, 24, 40), (2, 6, 10, 48, 80), (1, 5, 7, 13, 10),
             (1, 91, 100, 728, 800)]
# (N, hs, ws, fh, fw)
GATHER_CASES = [(3, 7, 13, 1, 1), (3, 7, 13, 2, 2), (3, 7, 13, 4, 4), (3, 7, 13, 8, 8), (2, 1, 9, 4, 4), (2, 6, 10, 3, 5),
                (2, 6, 10, 2, 4), (1, 725, 724, 1, 1), (1, 725, 724, 2, 2)]


def d2d_case(N, hs, ws, H, W):
    g = torch.Generator().manual_seed(hs * 100 + H)
    return torch.rand(N, 1, hs, ws, generator=g)


def ref_d2d(disp, H, W, dt):
    up = F.interpolate(disp.to(dt), size=(H, W), mode="bilinear", align_corners=False)
    return up, ol.disp_to_depth(up, MIN_D, MAX_D)[1]


def gather_case(N, hs, ws, fh, fw):
    g = torch.Generator().manual_seed(hs * 100 + ws + fh)
    return torch.randn(N, 1, hs * fh, ws * fw, generator=g), torch.randn(N, 1, hs, ws, generator=g)   # gup, prior contents


def ref_gather(gup, hs, ws, dt):
    d = torch.zeros(gup.shape[0], 1, hs, ws, dtype=dt, requires_grad=True)
    F.interpolate(d, size=gup.shape[2:], mode="bilinear", align_corners=False).backward(gup.to(dt))
    return d.grad


# ====================================================================================================== smoothness
SMOOTH_GEOMS = [(5, 3, 7), (3, 9, 29), (2, 2, 2), (2, 16, 24), (2, 5, 7), (1, 1040, 520)]
SMOOTH_W = 0.37                                            # wts[2] handed to pd_smooth_bwd


def smooth_case(N, h, w):
    """disp [N,1,h,w] on a 2^-10 lattice in (0.1, 0.95) (neighbours are equal or differ by >= 2^-10, far above the rounding
    of the normalisation), with constant patches (ties in x and in y); img [N,3,h,w] uniform."""
    g = torch.Generator().manual_seed(100 * h + w + N)
    yy, xx = _grid(h, w)
    d = torch.stack([0.5 + 0.3 * torch.sin(xx / 5.0 + n) * torch.cos(yy / 4.0) for n in range(N)])[:, None]
    d = d + 0.1 * torch.rand(N, 1, h, w, generator=g)
    d[:, :, h // 2:h // 2 + 3, w // 2:w // 2 + 3] = 0.40625 + 0.03125 * torch.arange(N, dtype=torch.float32).view(N, 1, 1, 1)
    d[:, :, 0, :2] = 0.75                                  # a tie on the first row, also in the 2 x 2 image
    d = torch.round(d * 1024.0) / 1024.0
    img = torch.rand(N, 3, h, w, generator=g)
    return d.contiguous(), img.contiguous()


def smooth_ties(d):
    return (d[:, :, :, 1:] == d[:, :, :, :-1]).sum().item(), (d[:, :, 1:, :] == d[:, :, :-1, :]).sum().item()


def ref_image_mean(disp, dt):
    return disp.to(dt).mean(dim=(1, 2, 3))


def ref_edge_weights(img, dt):
    """[N,h,w,2] = e^{-mean_c |dx I|}, e^{-mean_c |dy I|} (layers.py:459-463), 0 on the last column / row."""
    img = img.to(dt)
    N, _, h, w = img.shape
    e = torch.zeros(N, h, w, 2, dtype=dt)
    e[:, :, :-1, 0] = torch.exp(-torch.mean(torch.abs(img[:, :, :, :-1] - img[:, :, :, 1:]), 1))
    e[:, :-1, :, 1] = torch.exp(-torch.mean(torch.abs(img[:, :, :-1, :] - img[:, :, 1:, :]), 1))
    return e


def ref_smooth(disp, img, dt, normalise, w_sm=SMOOTH_W):
    """(sum_x, sum_y, loss, d (w_sm loss) / d disp): ol.get_smooth_loss on the mean-normalised (or raw) disparity."""
    d = disp.to(dt).clone().requires_grad_(True)
    img = img.to(dt)
    nd = d / (d.mean(2, True).mean(3, True) + 1e-7) if normalise else d
    loss = ol.get_smooth_loss(nd, img)
    (torch.tensor(w_sm, dtype=torch.float32).to(dt) * loss).backward()
    e = ref_edge_weights(img, dt)
    with torch.no_grad():
        sx = (torch.abs(nd[:, 0, :, :-1] - nd[:, 0, :, 1:]) * e[:, :, :-1, 0]).sum()
        sy = (torch.abs(nd[:, 0, :-1, :] - nd[:, 0, 1:, :]) * e[:, :-1, :, 1]).sum()
    return sx, sy, loss.detach(), d.grad


# ====================================================================================================== whole loss
def ms_case(N, H, W, zooms, seed=0):
    """One disparity and colour image per slot; the disparity of a slot is the smooth prediction surface sampled on its own
    grid (plus 1e-3 U), so that the upsampled depth is a surface, not white noise."""
    c = sup_case(N, H, W)
    g = torch.Generator().manual_seed(7 * H + W + seed)
    disps, colors = [], []
    for i, f in enumerate(zooms):
        hs, ws = H // f, W // f
        yy, xx = _grid(hs, ws)
        yy, xx = (yy + 0.5) * f - 0.5, (xx + 0.5) * f - 0.5
        if H > 256:          # tall: a sawtooth in y, see sup_case
            depth = torch.stack([0.75 + 0.92 * torch.frac(yy / 23.0 + 0.37 + 0.1 * n + 0.05 * i) + 0.1 * torch.sin(xx / 3.0) for n in range(N)])
        else:
            depth = torch.stack([1.05 + 0.4 * torch.sin(xx / 11.0 + 0.5 + 0.2 * i) * torch.cos(yy / 8.0 + 0.3 * n) for n in range(N)])
        d = ((1.0 / depth - 1.0 / MAX_D) / DISP_RANGE)[:, None] + (1e-4 if H > 256 else 1e-3) * torch.rand(N, 1, hs, ws, generator=g)
        disps.append(d.contiguous())
        colors.append(torch.rand(N, 3, hs, ws, generator=g))
    return dict(N=N, H=H, W=W, gt=c["gt"], K=c["K"], disps=disps, colors=colors, zooms=list(zooms),
                scale_ids=[int(math.log2(f)) for f in zooms])


MS_GVALS_HEAD = 1.7                                        # upstream gradient: 1.7 on vals[0], 1 on every other entry


def ref_multiscale(c, dt, w_normals=0.35, w_smooth=1e-3):
    """ol.compute_losses slot by slot -> (vals [1+3S], depths, d (1.7 vals[0] + sum vals[1:]) / d disp_s)."""
    S = len(c["disps"])
    gt, K = c["gt"].to(dt), c["K"].to(dt)
    dl = [d.to(dt).clone().requires_grad_(True) for d in c["disps"]]
    vals, depths = [None], []
    for i, sid in enumerate(c["scale_ids"]):
        depth = ol.upsample_disp_to_depth(dl[i], c["H"], c["W"], MIN_D, MAX_D)
        L = ol.compute_losses({"depth": gt, ("K", 0): K, ("color", 0, sid): c["colors"][i].to(dt)},
                              {("disp", sid): dl[i], ("depth", 0, sid): depth}, scales=[sid], min_depth=LO, max_depth=HI,
                              normals_loss_weight=w_normals, disparity_smoothness=w_smooth)
        vals += [L[f"loss/{sid}"], L[f"supervised_depth_loss/{sid}"], L[f"normals_loss/{sid}"]]
        depths.append(depth.detach())
    vals[0] = sum(vals[1::3]) / S
    vals = torch.stack(vals)
    (MS_GVALS_HEAD * vals[0] + vals[1:].sum()).backward()
    return vals.detach(), depths, [d.grad for d in dl]


# ====================================================================================================== bookkeeping
def ref_finalize(sup_part, sup_rows, sm_part, sm_rows, dims, scale_ids, w_normals, w_smooth):
    """trainer.py:1241-1265 on partial sums, fp64.  sup_part [S,stride,3], sm_part [S,stride,2] -> (sums [S*5], vals [1+3S])."""
    S = len(scale_ids)
    wn, wsm = float(torch.tensor(w_normals, dtype=torch.float32)), float(torch.tensor(w_smooth, dtype=torch.float32))
    sums, vals = [], [0.0]
    for s in range(S):
        a = [sup_part[s, :sup_rows[s], j].double().sum().item() for j in range(3)]
        a += [sm_part[s, :sm_rows[s], j].double().sum().item() for j in range(2)]
        N, h, w = dims[3 * s:3 * s + 3]
        l1, ln = a[0] / a[2], a[1] / a[2]
        smooth = a[3] / (N * h * (w - 1)) + a[4] / (N * (h - 1) * w)
        ls = l1 + wn * ln + wsm * smooth / 2 ** scale_ids[s]
        sums += a
        vals += [ls, l1, ln]
    vals[0] = sum(vals[1::3]) / S
    return torch.tensor(sums, dtype=torch.float64), torch.tensor(vals, dtype=torch.float64)


def ref_loss_weights(gvals, scale_ids, w_normals, w_smooth):
    """Per scale (w_L1, w_LN, w_sm): d loss / d (L1_s, LN_s, smooth_s) given the upstream gradient of vals; fp64 values and
    the magnitude sum of the terms each is made of (for the fp32 rounding bound)."""
    S = len(scale_ids)
    g = gvals.double()
    wn, wsm = float(torch.tensor(w_normals, dtype=torch.float32)), float(torch.tensor(w_smooth, dtype=torch.float32))
    out, mag = [], []
    for s in range(S):
        gl = g[0].item() / S + g[1 + 3 * s].item()
        glm = abs(g[0].item()) / S + abs(g[1 + 3 * s].item())
        out += [gl + g[2 + 3 * s].item(), gl * wn + g[3 + 3 * s].item(), gl * wsm / 2 ** scale_ids[s]]
        mag += [glm + abs(g[2 + 3 * s].item()), glm * wn + abs(g[3 + 3 * s].item()), glm * wsm / 2 ** scale_ids[s]]
    return torch.tensor(out, dtype=torch.float64), torch.tensor(mag, dtype=torch.float64)


def finalize_case(S, rows, stride, scale_ids, seed=0):
    """Synthetic partial rows (positive, counts integral) with NaN in the rows beyond the row count."""
    g = torch.Generator().manual_seed(S * 10000 + rows + seed)
    sup = torch.full((S, stride, 3), float("nan"))
    sm = torch.full((S, stride, 2), float("nan"))
    sup_rows = [max(1, rows - s) for s in range(S)]
    sm_rows = [max(1, (rows >> s)) for s in range(S)]
    dims = []
    for s in range(S):
        sup[s, :sup_rows[s], :2] = 50.0 * torch.rand(sup_rows[s], 2, generator=g)
        sup[s, :sup_rows[s], 2] = torch.randint(1, 257, (sup_rows[s],), generator=g).float()
        sm[s, :sm_rows[s]] = 20.0 * torch.rand(sm_rows[s], 2, generator=g)
        dims += [2 + s, 64 >> min(s, 4), 96 >> min(s, 4)]
    return sup, sup_rows, sm, sm_rows, dims


# ====================================================================================================== predicted normals
NPRED_CASES = [(3, 6, 10, 3, 4), (3, 6, 10, 5, 3), (1, 32808, 16, 3, 5)]      # (N, H, W, ld, ld_dpred)
NPRED_GOUT = 1.3


def npred_case(N, H, W):
    """sup_case with image 1 (if any) wholly out of range, and a predicted normal map [N,3,H,W] of norm in (0.5, 1.5)."""
    c = sup_case(N, H, W, dead_image=1 if N > 1 else None)
    g = torch.Generator().manual_seed(H + W)
    v = F.normalize(torch.randn(N, 3, H, W, generator=g), dim=1)
    c["normals"] = (v * (0.5 + torch.rand(N, 1, H, W, generator=g))).contiguous()
    return c


def ref_npred(c, dt):
    """(loss, count, d (1.3 loss) / d normals [N,3,H,W])."""
    p = c["normals"].to(dt).clone().requires_grad_(True)
    loss = ol.normals_pred_loss(p, c["gt"].to(dt), c["K"].to(dt), LO, HI)
    (torch.tensor(NPRED_GOUT, dtype=torch.float32).to(dt) * loss).backward()
    return loss.detach(), ((c["gt"] >= LO) & (c["gt"] <= HI)).sum().item(), p.grad


# ====================================================================================================== depth metrics
METRIC_CASES = ["bounds", "one_pixel_by_mask", "p1", "stride_loop"]


def metrics_case(name):
    """gt, pred [N,P] and (mask, mask_value) or (None, 0).  gt holds float32(0.1) and float32(2.0) exactly (excluded: the
    bounds are exclusive here), predictions lie outside the range too (clamped first, trainer.py:1422-1423)."""
    g = torch.Generator().manual_seed(len(name))
    N, P = {"bounds": (3, 700), "one_pixel_by_mask": (2, 300), "p1": (2, 1), "stride_loop": (2, 64 * 256 * 2 + 3)}[name]
    gt = 0.05 + 2.2 * torch.rand(N, P, generator=g)
    pred = (gt * (0.6 + 0.9 * torch.rand(N, P, generator=g))).clamp(0.02, 3.0)
    mask, mask_value = None, 0
    if name == "p1":
        gt = torch.tensor([[0.8], [1.7]])
        pred = torch.tensor([[2.6], [1.5]])
    else:
        gt[:, 5::37] = LO
        gt[:, 11::41] = HI
        pred[:, 3::29] = 0.03
        pred[:, 7::31] = 2.7
    if name == "one_pixel_by_mask":
        mask = (torch.randint(0, 5, (N, P), generator=g) * 20).int()
        gt[:, 123] = 1.25
        mask[:, 123] = 160
        mask_value = 160
    elif name == "stride_loop":
        mask = (torch.randint(0, 3, (N, P), generator=g) * 80).int()
        mask_value = 80
    return gt.contiguous(), pred.contiguous(), mask, mask_value


def ref_metrics(gt, pred, mask, mask_value, dt):
    """[N,8]: ol.compute_depth_errors on the selected pixels of every image, and their number."""
    out = []
    for n in range(gt.shape[0]):
        sel = (gt[n] > LO) & (gt[n] < HI)
        if mask is not None:
            sel = sel & (mask[n] == mask_value)
        p = pred[n][sel].to(dt).clamp(torch.tensor(LO).to(dt), torch.tensor(HI).to(dt))
        out.append(torch.stack(list(ol.compute_depth_errors(gt[n][sel].to(dt), p)) + [sel.sum().to(dt)]))
    return torch.stack(out)
