"""Polarimetric depth refinement on the device (pd_polar_refine_*, csrc/polar_refine.hip).

``polar_normals_stats(maps=True)`` lets a coarse depth resolve the pi and the diffuse / specular ambiguity of the polarisation
normals and returns the winner per pixel.  ``polar_refine`` takes the step after it: it integrates those normals back into the
depth that disambiguated them.  The depth supplies the low frequencies and fixes the ambiguities, the polarisation supplies
the fine relief.  Per item it is a screened Poisson problem in zeta = log z on the pixel grid,

    E = sum_pixels lam (zeta - zeta0)^2 + sum_edges w (zeta_b - zeta_a - g)^2,    w = sqrt(rho_a rho_b),

whose edge gradients g come from the normals and the viewing rays, solved by ``iters`` steps of Chebyshev semi-iteration on the
Jacobi-preconditioned normal equations: no inner products, hence bit-reproducible, no host synchronisation, capturable.  The
definition is the header's (include/polardepth.h); tests/polar_refine_ref.py states it in NumPy.

The prior need not be trusted equally everywhere: lam becomes lam_i = lam * clamp(weight_i) per pixel, from a ready map, from the
Laplace scale the decoder's uncertainty head states, and from the previous round's solution (a Huber data term by iteratively
reweighted least squares).  lam_i enters the diagonal, the right-hand side and the spectrum bound; the steps are the same launches
(pd_polar_refine_setup_w, _table_w, _weights; tests/polar_refine_w_ref.py)."""
import math
from collections import namedtuple

import torch

from ._lib import lib, check, ptr, stream_ptr
from ._records import need_cuda

PolarRefined = namedtuple("PolarRefined", "depth residual touched choice")
PolarRefined.__doc__ = """What ``polar_refine`` returns: ``depth`` fp32 in the shape of the prior, ``residual`` fp64 [N] (the
largest Jacobi residual |r| in log depth after the last step), ``touched`` uint8 [N,H,W] (1 where a live edge reaches the pixel;
everywhere else ``depth`` holds the prior's bits), ``choice`` uint8 [N,H,W] (``polar_normals_eval.CHOICE_NAMES``; None with
``normals=``)."""


def _check_solver_args(lam, iters, edge_max, incidence_max_deg, rounds):
    if not (isinstance(lam, (int, float)) and math.isfinite(lam) and lam > 0):
        raise ValueError(f"lam must be finite and > 0, got {lam!r}")
    if not (isinstance(iters, int) and not isinstance(iters, bool) and iters >= 1):
        raise ValueError(f"iters must be an integer >= 1, got {iters!r}")
    if not (isinstance(edge_max, (int, float)) and math.isfinite(edge_max) and edge_max >= 0):
        raise ValueError(f"edge_max must be finite and >= 0, got {edge_max!r}")
    if not (isinstance(incidence_max_deg, (int, float)) and math.isfinite(incidence_max_deg) and 0 <= incidence_max_deg < 90):
        raise ValueError(f"incidence_max_deg must be in [0, 90), got {incidence_max_deg!r}")
    if not (isinstance(rounds, int) and not isinstance(rounds, bool) and rounds >= 1):
        raise ValueError(f"rounds must be an integer >= 1, got {rounds!r}")


def _dolp_pitch(xolp, H, W):
    """(xolp, ldp): read in place where the rows are dense in x and the planes and items lie at their pitch, else a copy."""
    s = xolp.stride()
    ldp = s[2] if H > 1 else W
    if (xolp.dtype == torch.float32 and s[3] == 1 and ldp >= W and s[1] == H * ldp and
            (xolp.shape[0] == 1 or s[0] == 2 * H * ldp) and xolp.data_ptr() % 4 == 0):
        return xolp, ldp
    return xolp.float().contiguous(), W


MAX_FUSED_STEPS = 8                 # PD_POLAR_REFINE_MAX_T
FUSED_STEPS = 4                     # steps per launch of the default route (DESIGN.md, section 4 has the measurement); 0 = one each


def solve(depth, K, pol_normal, xolp, ldp, valid, lam, iters, edge_max, incidence_max_deg, fused=None, weight=None,
          weight_min=1 / 16, weight_max=1.0, zeta0_out=None):
    """setup -> table -> ``iters`` steps -> finish on contiguous fp32 ``depth`` [N,H,W], ``K`` [N,4,4], ``pol_normal`` [N,H,W,4],
    ``xolp`` [N,2,H,ldp], ``valid`` uint8 [N,H,W] or None -> (depth_out, residual, touched, zeta), zeta fp64 [N,H,W] the
    solution in log depth (zeta0 where nothing is touched).  ``fused``: T in 1 .. 8 = pd_polar_refine_steps, T steps per launch
    (the last launch takes what is left); 0 = pd_polar_refine_step, one launch per step; None = FUSED_STEPS.  Both routes
    return the same bits.  2 + ceil(iters / T) + 2 launches.  ``weight``: contiguous fp32 [N,H,W], the per-pixel weight of the
    prior, clamped to [``weight_min``, ``weight_max``]: pd_polar_refine_setup_w and _table_w take the place of _setup and
    _table, the steps and finish are the same launches; None calls exactly what it called before there was a weight.
    ``zeta0_out``: a contiguous fp64 [N,H,W] tensor that setup writes the prior's log depth into (the reweighting of a robust
    round reads it)."""
    fused = FUSED_STEPS if fused is None else int(fused)
    if not 0 <= fused <= MAX_FUSED_STEPS:
        raise ValueError(f"fused must be in [0, {MAX_FUSED_STEPS}], got {fused!r}")
    N, H, W = depth.shape
    dev = depth.device
    out = torch.empty_like(depth)
    residual = torch.zeros(N, dtype=torch.float64, device=dev)
    touched = torch.zeros((N, H, W), dtype=torch.uint8, device=dev)
    if N == 0 or H == 0 or W == 0:
        return out, residual, touched, torch.empty((N, H, W), dtype=torch.float64, device=dev)
    f64 = lambda *shape: torch.empty(shape, dtype=torch.float64, device=dev)
    zeta0 = f64(N, H, W) if zeta0_out is None else zeta0_out
    coef, za, zb, d = f64(N, 4, H, W), f64(N, H, W), f64(N, H, W), f64(N, H, W)
    S, table = f64(N), f64(N, iters, 2)
    ws = torch.empty(int(lib.pd_polar_refine_workspace(N, H, W)), dtype=torch.uint8, device=dev)
    cos_inc = math.cos(math.radians(float(incidence_max_deg)))
    with torch.cuda.device(dev):
        st = stream_ptr()
        if weight is None:
            check(lib.pd_polar_refine_setup(ptr(depth), ptr(K), ptr(pol_normal), ptr(xolp), ldp, ptr(valid), float(lam),
                                            float(edge_max), cos_inc, ptr(zeta0), ptr(coef), None, ptr(ws), ws.numel(), N, H, W, st),
                  "pd_polar_refine_setup")
            check(lib.pd_polar_refine_table(ptr(ws), ws.numel(), float(lam), iters, ptr(S), ptr(table), N, H, W, st),
                  "pd_polar_refine_table")
        else:                               # S holds A, the lower end of the spectrum
            check(lib.pd_polar_refine_setup_w(ptr(depth), ptr(K), ptr(pol_normal), ptr(xolp), ldp, ptr(valid), float(lam),
                                              float(edge_max), cos_inc, ptr(weight), float(weight_min), float(weight_max), ptr(zeta0),
                                              ptr(coef), None, ptr(ws), ws.numel(), N, H, W, st), "pd_polar_refine_setup_w")
            check(lib.pd_polar_refine_table_w(ptr(ws), ws.numel(), iters, ptr(S), ptr(table), N, H, W, st),
                  "pd_polar_refine_table_w")
        src, dst = zeta0, za
        if fused:
            d_in, d_out = None, d
            for k in range(0, iters, fused):
                check(lib.pd_polar_refine_steps(ptr(coef), ptr(table), iters, k, min(fused, iters - k), ptr(src), ptr(dst),
                                                ptr(d_in), ptr(d_out), N, H, W, st), "pd_polar_refine_steps")
                src, dst = dst, (zb if dst is za else za)
                d_in, d_out = d_out, (f64(N, H, W) if d_in is None else d_in)
        else:
            for k in range(iters):
                check(lib.pd_polar_refine_step(ptr(coef), ptr(table), iters, k, ptr(src), ptr(dst), ptr(d), N, H, W, st),
                      "pd_polar_refine_step")
                src, dst = dst, (zb if dst is za else za)
        check(lib.pd_polar_refine_finish(ptr(depth), ptr(coef), ptr(src), ptr(out), ptr(touched), ptr(residual), ptr(ws),
                                         ws.numel(), N, H, W, st), "pd_polar_refine_finish")
    return out, residual, touched, src


def _check_weight_args(unc_ref, robust, weight_min, weight_max, rounds):
    num = lambda v: isinstance(v, (int, float)) and not isinstance(v, bool)
    if not (num(unc_ref) and math.isfinite(unc_ref) and unc_ref > 0):
        raise ValueError(f"unc_ref must be finite and > 0, got {unc_ref!r}")
    if not (num(weight_min) and num(weight_max) and 0 < weight_min <= weight_max < math.inf):
        raise ValueError(f"the clamp must be 0 < weight_min <= weight_max < inf, got weight_min = {weight_min!r}, weight_max = "
                         f"{weight_max!r}")
    if robust is not None:
        if not (num(robust) and math.isfinite(robust) and robust > 0):
            raise ValueError(f"robust must be None or a finite threshold > 0 in log depth, got {robust!r}")
        if rounds < 2:
            raise ValueError(f"robust reweights from the previous round's solution: it needs rounds >= 2, got rounds = {rounds}")


def weights(depth, uncertainty=None, unc_ref=0.002, zeta_prev=None, zeta0=None, robust=None):
    """pd_polar_refine_weights: the raw weight map fp32 [N,H,W] = (float)(u * h) from contiguous fp32 ``depth`` [N,H,W] --
    u = ((unc_ref z) / b)^2 with ``uncertainty`` = b, fp32 [N,H,W] in metres (1 without), h = min(1, robust / |zeta_prev - zeta0|)
    with the fp64 [N,H,W] pair (1 without).  One launch, capturable."""
    N, H, W = depth.shape
    out = torch.empty((N, H, W), dtype=torch.float32, device=depth.device)
    if out.numel() == 0:
        return out
    with torch.cuda.device(depth.device):
        check(lib.pd_polar_refine_weights(ptr(depth), ptr(uncertainty), float(unc_ref), ptr(zeta_prev), ptr(zeta0),
                                          0.0 if robust is None else float(robust), ptr(out), N, H, W, stream_ptr()),
              "pd_polar_refine_weights")
    return out


def polar_refine(depth, K, pol_normals, xolp, valid=None, lam=0.02, iters=100, edge_max=0.05, incidence_max_deg=80.0,
                 rho_min=0.05, rho_max=1.0, aolp_sign=1, ray_frame=False, rounds=1, normals=None, weight=None, uncertainty=None,
                 unc_ref=0.002, robust=None, weight_min=1 / 16, weight_max=1.0, return_weight=False):
    """Refine ``depth`` with the polarisation normals -> ``PolarRefined``.

    depth         [N,1,H,W] or [N,H,W] fp32, the prior.  A pixel whose prior is not finite or not positive keeps its bits
    K             [N,4,4] intrinsics
    pol_normals   [N,9,H,W] fp32, K1's three candidates (``polar_forward``'s "normals"); not read with ``normals=``
    xolp          [N,2,H,W] fp32; channel 0 (DoLP) weights the edges.  A view with padded rows is read in place
    valid         [N,1,H,W] or [N,H,W] bool / uint8 or None: a 0 takes the pixel out of the solve
    lam           the weight of the prior against the normals; smaller follows the normals further
    iters         Chebyshev steps (FUSED_STEPS of them per launch)
    edge_max      the largest step of the PRIOR in log depth across which normals are integrated; beyond it an edge is cut,
                  so a depth discontinuity of the prior is kept
    incidence_max_deg   a normal further than this from its viewing ray takes its pixel out (p, q diverge at 90 degrees)
                  lam = 0.02, iters = 100, edge_max = 0.05 and incidence_max_deg = 80 are CONVENTIONS, not measurements, as
                  rho_min = 0.05 is
    rho_min, rho_max, aolp_sign, ray_frame   passed to ``polar_normals_stats``, which disambiguates the candidates against
                  the normals of the depth
    rounds        > 1: disambiguate again against the refined depth and solve again, always from the original prior
    normals       a ready [N,H,W,4] fp32 normal map (zeros = no normal): the disambiguation is skipped, ``choice`` is None

    The weight of the prior per pixel, lam_i = lam * clamp(weight_i, weight_min, weight_max); the three sources multiply, and
    with none of them the call is the scalar one, launch for launch:
    weight        [N,1,H,W] or [N,H,W]: a ready map, any values (a NaN, a zero, a negative take ``weight_min``)
    uncertainty   [N,1,H,W] or [N,H,W]: the Laplace scale b in metres that the decoder states for ``depth``
                  (``predict_all``'s "uncertainty"): u = ((unc_ref z) / b)^2, so a pixel whose stated relative scale b / z is
                  ``unc_ref`` has the weight 1, one that states twice as much a quarter.  A regional bias that the network
                  knows of is then bridged by the normals while the good pixels hold
    robust        c, a threshold in log depth: a Huber data term by iteratively reweighted least squares.  The first round has
                  h = 1, every later round h = min(1, c / |zeta - zeta0|) from the previous round's solution, and solves from
                  the original prior as ``rounds`` always does.  It needs ``rounds >= 2``.  0.005 is a fair start
    weight_min, weight_max   the clamp.  The lower end of the solver's spectrum is a >= lam weight_min / (lam weight_min +
                  4 rho_max): a smaller ``weight_min`` therefore needs more ``iters``; ``residual`` tells
                  unc_ref = 0.002, weight_min = 1/16 and robust's 0.005 are CONVENTIONS, not measurements
    return_weight True: -> (``PolarRefined``, weight), the raw (unclamped) fp32 [N,H,W] map of the last round, None where no
                  source was given"""
    from .polar_normals_eval import polar_normals_stats
    from ._records import frames
    need_cuda("polar_refine", depth, K, pol_normals, xolp, valid, normals, weight, uncertainty)
    _check_solver_args(lam, iters, edge_max, incidence_max_deg, rounds)
    _check_weight_args(unc_ref, robust, weight_min, weight_max, rounds)
    shape = tuple(depth.shape)
    if depth.dim() == 4 and depth.shape[1] == 1:
        prior = depth[:, 0]
    elif depth.dim() == 3:
        prior = depth
    else:
        raise ValueError(f"depth must be [N,1,H,W] or [N,H,W], got {shape}")
    N, H, W = prior.shape
    if tuple(K.shape) != (N, 4, 4):
        raise ValueError(f"K must be [{N},4,4], got {tuple(K.shape)}")
    if tuple(xolp.shape) != (N, 2, H, W):
        raise ValueError(f"xolp must be {(N, 2, H, W)}, got {tuple(xolp.shape)}")
    if normals is None and (pol_normals is None or tuple(pol_normals.shape) != (N, 9, H, W)):
        raise ValueError(f"pol_normals must be {(N, 9, H, W)}, got {None if pol_normals is None else tuple(pol_normals.shape)}")
    if normals is not None and tuple(normals.shape) != (N, H, W, 4):
        raise ValueError(f"normals must be {(N, H, W, 4)}, got {tuple(normals.shape)}")
    prior = prior.float().contiguous()
    Km = K.float().contiguous()
    v8 = None if valid is None else frames(valid, "valid", N, H, W).ne(0).to(torch.uint8).contiguous()
    given = None if weight is None else frames(weight, "weight", N, H, W).float().contiguous()
    b = None if uncertainty is None else frames(uncertainty, "uncertainty", N, H, W).float().contiguous()
    dolp, ldp = _dolp_pitch(xolp, H, W)
    zeta0 = None if robust is None else torch.empty((N, H, W), dtype=torch.float64, device=prior.device)
    choice, cur, zeta, wmap = None, prior, None, None
    for _ in range(rounds):
        if normals is not None:
            pn = normals.float().contiguous()
        else:
            st = polar_normals_stats(cur[:, None], pol_normals, xolp, K=Km, valid=v8, classes=(("all", None),), rho_min=rho_min,
                                     rho_max=rho_max, aolp_sign=aolp_sign, maps=True, ray_frame=ray_frame)
            pn, choice = st.pol_normal, st.choice
        wmap = given
        if b is not None or zeta is not None:                   # zeta: the previous round's solution, kept only for ``robust``
            wmap = weights(prior, b, unc_ref, zeta, None if zeta is None else zeta0, robust)
            if given is not None:
                wmap = given * wmap
        cur, residual, touched, z = solve(prior, Km, pn, dolp, ldp, v8, lam, iters, edge_max, incidence_max_deg, weight=wmap,
                                          weight_min=weight_min, weight_max=weight_max, zeta0_out=zeta0)
        zeta = z if robust is not None else None
    out = PolarRefined(cur.reshape(shape), residual, touched, choice)
    return (out, wmap) if return_weight else out
