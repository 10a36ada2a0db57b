"""The disparity-head kernels of csrc/disphead.hip through the C ABI (pd_disphead_fwd / _bwd_data / _bwd_weight / _bwd), so that y, add,
elu, accumulate and the NULL arguments are the test's to choose.  tests/disphead_cases.py holds the rows, the data and the NumPy fp64
reference; tests/test_disphead_cases.py proves on the CPU that each row's data is exactly summable and that the rows reach every
kernel in every regime (borders, tile edges, ragged tails, a second pass of every grid-stride loop, every slice count of the reduce
kernel).

  exact class    gradients torch.equal to the fp32 rounding of the reference, from both routes and with every option of the fused
                 entry point; the forward within the sigmoid's own rounding, |y - y_ref| <= (E + 2) 2^-24 y_ref elementwise, where
                 E = 2 stands for expf (the HIP math documentation with its table of ulp errors is not part of the ROCm install: the
                 fallback value) and + 2 for the addition and the correctly rounded division
  random class   elementwise against fp64 with u = 2^-24:  forward 0.25 (9C + 2) u sum|x w| + (E + 2) u y_ref;  dx (T + 3) u sum|dz w|
                 with T the element's number of terms;  dw, db (P + 2) u sum_p|dz x| with P = N H W, the bound of any summation order;
                 dz formed in fp64 from the fp32 y the kernel received.  Two calls return the same bits.
Every output buffer has 64 NaN guard floats in front and behind, which must keep their bits; the workspace is filled with NaN before
every call, so a slice that is read without having been written shows.

Measured on the MI355X (max of err / bound over all rows): see MEASURED below and DESIGN.md."""
import ctypes

import numpy as np
import pytest
import torch

import disphead_cases as dc
from polardepth._lib import lib, stream_ptr

pytestmark = pytest.mark.gpu
torch.set_num_threads(min(16, torch.get_num_threads()))
GUARD = 64
E = dc.EXPF_ULP
U = dc.U
# max err / bound over all rows as these tests print it, on the MI355X (a record, asserted nowhere)
MEASURED = {"forward, exact class": 0.363, "forward, random class": 0.007, "dx (either route)": 0.532,
            "dw: bwd_weight / bwd": (0.353, 0.312), "db: bwd_weight / bwd": (0.146, 0.121)}


class Out:
    """n floats between two guard bands of NaN; `fill`: initial contents (default NaN)."""

    def __init__(self, n, fill=None):
        self.n = n
        self.buf = torch.full((n + 2 * GUARD,), float("nan"), dtype=torch.float32, device="cuda")
        if fill is not None:
            self.body.copy_(fill)
        self.before = self.buf.view(torch.int32).clone()

    @property
    def body(self):
        return self.buf[GUARD:GUARD + self.n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.buf.data_ptr() + 4 * GUARD)

    def np(self, shape=None):
        a = self.body.cpu().numpy()
        return a if shape is None else a.reshape(shape)

    def guards_intact(self, what):
        now = self.buf.view(torch.int32)
        ok = torch.equal(now[:GUARD], self.before[:GUARD]) and torch.equal(now[GUARD + self.n:], self.before[GUARD + self.n:])
        assert ok, f"{what}: a guard element changed"

    def untouched(self, what):
        assert torch.equal(self.buf.view(torch.int32), self.before), f"{what}: written to"


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).cuda()


def p(t):
    return None if t is None else (t.ptr if isinstance(t, Out) else ctypes.c_void_p(t.data_ptr()))


def ok(rc, what):
    assert rc == 0, f"{what}: {rc} {lib.pd_last_error()}"


def workspace(C):
    return torch.full((lib.pd_disphead_workspace(C),), 255, dtype=torch.uint8, device="cuda")       # every float a NaN


def run_fwd(x, w, b, shape):
    N, C, H, W = shape
    y = Out(N * H * W)
    ok(lib.pd_disphead_fwd(p(x), p(w), p(b), p(y), N, H, W, C, stream_ptr()), "pd_disphead_fwd")
    torch.cuda.synchronize()
    y.guards_intact(f"pd_disphead_fwd {shape} y")
    return y


def run_bwd_data(dy, y, w, shape):
    N, C, H, W = shape
    dx = Out(N * H * W * C)
    ok(lib.pd_disphead_bwd_data(p(dy), p(y), p(w), p(dx), N, H, W, C, stream_ptr()), "pd_disphead_bwd_data")
    torch.cuda.synchronize()
    dx.guards_intact(f"pd_disphead_bwd_data {shape} dx")
    return dx


def run_bwd_weight(dy, y, x, shape, accumulate=0, dw=None, db=None, no_db=False):
    N, C, H, W = shape
    dw = dw or Out(9 * C)
    db = db or Out(1)
    ws = workspace(C)
    ok(lib.pd_disphead_bwd_weight(p(dy), p(y), p(x), p(dw), None if no_db else p(db), p(ws), ws.numel(), N, H, W, C, accumulate,
                                  stream_ptr()), "pd_disphead_bwd_weight")
    torch.cuda.synchronize()
    dw.guards_intact(f"pd_disphead_bwd_weight {shape} dw")
    db.guards_intact(f"pd_disphead_bwd_weight {shape} db")
    return dw, db


def run_bwd(dy, y, x, w, shape, add=None, elu=0, accumulate=0, dw=None, db=None, no_dx=False, no_db=False):
    N, C, H, W = shape
    dx = Out(N * H * W * C)
    dw = dw or Out(9 * C)
    db = db or Out(1)
    ws = workspace(C)
    ok(lib.pd_disphead_bwd(p(dy), p(y), p(x), p(w), p(add), elu, None if no_dx else p(dx), p(dw), None if no_db else p(db), p(ws),
                           ws.numel(), N, H, W, C, accumulate, stream_ptr()), "pd_disphead_bwd")
    torch.cuda.synchronize()
    for name, o in (("dx", dx), ("dw", dw), ("db", db)):
        o.guards_intact(f"pd_disphead_bwd {shape} {name}")
    return dx, dw, db


def exact(got, ref, what):
    """got: fp32 array; ref: fp64.  Equal bits, or the first difference."""
    ref = np.asarray(ref, dtype=np.float64).astype(np.float32).reshape(got.shape)
    if not np.array_equal(got, ref):         # (a NaN in got differs from everything)
        bad = ~(got == ref)
        k = int(np.argmax(bad))
        idx = tuple(int(i) for i in np.unravel_index(k, got.shape))
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} elements differ; first at {idx}: got {got.flat[k]!r} ref {ref.flat[k]!r}")


def within(got, ref, bound, what):
    """|got - ref| <= bound elementwise; prints and returns max err / bound."""
    got = np.asarray(got, dtype=np.float64).reshape(np.shape(ref))
    err = np.abs(got - ref)
    ratio = np.where(err == 0, 0.0, err / np.maximum(bound, 1e-300))
    worst = float(np.max(ratio)) if np.isfinite(got).all() else float("inf")
    print(f"{what}: max err / bound = {worst:.3f}")
    if not worst <= 1.0:
        k = int(np.argmax(np.where(np.isfinite(ratio), ratio, np.inf)))
        idx = tuple(int(i) for i in np.unravel_index(k, np.shape(ref))) if np.ndim(ref) else ()
        raise AssertionError(f"{what}: {int((ratio > 1).sum())} of {ratio.size} elements over the bound; worst at {idx}: got {np.ravel(got)[k]!r} "
                             f"ref {np.ravel(ref)[k]!r} err {np.ravel(err)[k]:.3e} bound {np.ravel(np.broadcast_to(bound, np.shape(ref)))[k]:.3e}")
    return worst


def sigmoid_bound(y_ref):
    return (E + 2) * U * y_ref


SMALL_BWD = dc.shapes((dc.BWD, dc.BWD_DATA, dc.BWD_WEIGHT))
SMALL_FWD = dc.shapes((dc.FWD,))
BIG = [r for r in dc.ROWS if r.big]
RANDOM_SHAPES = dc.shapes(dc.ENTRIES, regimes=("border", "tile edge")) + [
    (4097, 16, 2, 2),        # second pass: tile forward <4>, fused backward <4>
    (1025, 128, 2, 2),       # ... fused backward <32>
    (1, 64, 50, 328),        # ... weight gradient <16>
]


# ====================================================================================================== exact gradients
@pytest.mark.parametrize("shape", SMALL_BWD, ids=dc.sid)
def test_gradients_bit_exact(shape):
    """dx, dw, db of pd_disphead_bwd_data + pd_disphead_bwd_weight and of pd_disphead_bwd with each of its options: torch.equal to the
    fp32 rounding of the fp64 reference (hence to each other)."""
    N, C, H, W = shape
    rows = dc.rows_of(shape)
    assert all(r.options == dc.OPTIONS[e] for e, r in rows.items())         # the options a row lists are the calls made below
    d = dc.case(shape, "exact")
    x, w, y, dy, add = (dev(d[k]) for k in ("x", "w", "y", "dy", "add"))
    keep = [(k, t, t.clone()) for k, t in (("x", x), ("w", w), ("y", y), ("dy", dy), ("add", add))]
    ref = d["bwd"]
    tag = dc.sid(shape)
    g = np.random.default_rng(N + C)
    dw0, db0 = g.integers(-8, 9, 9 * C).astype(np.float32), g.integers(-8, 9, 1).astype(np.float32)

    if dc.BWD_DATA in rows:
        exact(run_bwd_data(dy, y, w, shape).np(), ref["dx"], f"{tag} bwd_data dx")
    if dc.BWD_WEIGHT in rows:
        dw, db = run_bwd_weight(dy, y, x, shape)                                             # accumulate = 0 over NaN
        exact(dw.np(), ref["dw"], f"{tag} bwd_weight dw")
        exact(db.np(), ref["db"], f"{tag} bwd_weight db")
        dw, db = run_bwd_weight(dy, y, x, shape, 1, Out(9 * C, dev(dw0)), Out(1, dev(db0)))
        exact(dw.np(), ref["dw"].ravel() + dw0, f"{tag} bwd_weight dw accumulate")
        exact(db.np(), ref["db"] + db0, f"{tag} bwd_weight db accumulate")
        dw, db = run_bwd_weight(dy, y, x, shape, no_db=True)
        exact(dw.np(), ref["dw"], f"{tag} bwd_weight dw (dbias NULL)")
        db.untouched(f"{tag} bwd_weight db (dbias NULL)")
    if dc.BWD in rows:
        dx, dw, db = run_bwd(dy, y, x, w, shape)                                             # accumulate = 0 over NaN
        exact(dx.np(), ref["dx"], f"{tag} bwd dx")
        exact(dw.np(), ref["dw"], f"{tag} bwd dw")
        exact(db.np(), ref["db"], f"{tag} bwd db")
        for key, a, elu in (("bwd+add", add, 0), ("bwd+add+elu", add, 1), ("bwd+elu", None, 1)):
            dx, dw, db = run_bwd(dy, y, x, w, shape, add=a, elu=elu)
            exact(dx.np(), d[key]["dx"], f"{tag} {key} dx")
            exact(dw.np(), ref["dw"], f"{tag} {key} dw")
            exact(db.np(), ref["db"], f"{tag} {key} db")
        dx, dw, db = run_bwd(dy, y, x, w, shape, no_dx=True)
        dx.untouched(f"{tag} bwd dx (dx NULL)")
        exact(dw.np(), ref["dw"], f"{tag} bwd dw (dx NULL)")
        exact(db.np(), ref["db"], f"{tag} bwd db (dx NULL)")
        dx, dw, db = run_bwd(dy, y, x, w, shape, no_db=True)
        exact(dx.np(), ref["dx"], f"{tag} bwd dx (dbias NULL)")
        exact(dw.np(), ref["dw"], f"{tag} bwd dw (dbias NULL)")
        db.untouched(f"{tag} bwd db (dbias NULL)")
        dx, dw, db = run_bwd(dy, y, x, w, shape, accumulate=1, dw=Out(9 * C, dev(dw0)), db=Out(1, dev(db0)))
        exact(dx.np(), ref["dx"], f"{tag} bwd dx accumulate")
        exact(dw.np(), ref["dw"].ravel() + dw0, f"{tag} bwd dw accumulate")
        exact(db.np(), ref["db"] + db0, f"{tag} bwd db accumulate")
    for k, t, t0 in keep:
        assert torch.equal(t, t0), f"{tag}: operand {k} changed"


@pytest.mark.parametrize("row", [r for r in BIG if r.entry == dc.BWD_DATA], ids=lambda r: r.id)
def test_data_gradient_second_pass_bit_exact(row):
    """Just over 16384 * 4 * PPW pixels: the second iteration of the data gradient's grid-stride loop (a 64 MiB dx)."""
    d = dc.exact_inputs(row.shape, need_x=False)
    ref = dc.big_dx(d["w"], d["y"], d["dy"])["dx"].float()
    dx = run_bwd_data(dev(d["dy"]), dev(d["y"]), dev(d["w"]), row.shape)
    got = dx.body.view(ref.shape).cpu()
    if not torch.equal(got, ref):
        bad = (got != ref).nonzero()
        raise AssertionError(f"{row.id}: {bad.shape[0]} elements differ; first at {tuple(bad[0].tolist())}")


# ====================================================================================================== forward, exact inputs
@pytest.mark.parametrize("shape", SMALL_FWD, ids=dc.sid)
def test_forward_on_exact_inputs(shape):
    """z is exact, only the sigmoid rounds: |y - y_ref| <= (E + 2) 2^-24 y_ref, with and without bias."""
    d = dc.case(shape, "exact")
    x, w = dev(d["x"]), dev(d["wf"])
    b = dev(np.array([d["b"]]))
    N, C, H, W = shape
    for key, bias in (("fwd", b), ("fwd0", None)):
        y = run_fwd(x, w, bias, shape).np((N, H, W))
        within(y, d[key]["y"], sigmoid_bound(d[key]["y"]), f"{dc.sid(shape)} forward, exact class ({'bias' if bias is not None else 'bias NULL'})")


@pytest.mark.parametrize("row", [r for r in BIG if r.entry == dc.FWD], ids=lambda r: r.id)
def test_direct_forward_second_pass(row):
    """Just over 16384 * 4 * PPW pixels: the second iteration of the direct forward's grid-stride loop (a 64 MiB x), exact inputs."""
    N, C, H, W = row.shape
    d = dc.exact_inputs(row.shape)
    ref = dc.big_forward(d["x"], d["wf"], d["b"])
    assert np.abs(ref["z"]).max() <= 75 and ref["z_abs"].max() * 4 < 2 ** 24
    y = run_fwd(dev(d["x"]), dev(d["wf"]), dev(np.array([d["b"]])), row.shape).np((N, H, W))
    within(y, ref["y"], sigmoid_bound(ref["y"]), f"{row.id} forward, exact class")


@pytest.mark.parametrize("hw", [(2, 2), (3, 3), (4, 5), (9, 65), (17, 129)], ids=lambda hw: f"{hw[0]}x{hw[1]}")
def test_forward_forms_agree_bit_for_bit(hw):
    """The same 16-channel exact input zero-extended to 32, 64 and 128 channels (zero weights there) has the same exact z: the y of the
    tile form (16, 32) and of the direct form (64, 128) must be equal bits, whatever expf's error."""
    H, W = hw
    shape = (2, 16, H, W)
    d = dc.case(shape, "exact")
    b = dev(np.array([d["b"]]))
    ys = {}
    for C in dc.WIDTHS:
        x, w = np.zeros((2, H, W, C)), np.zeros((3, 3, C))
        x[..., :16], w[..., :16] = d["x"], d["wf"]
        x[..., 16:] = 0.5                                    # read, multiplied by a zero weight
        ys[C] = run_fwd(dev(x), dev(w), b, (2, C, H, W)).np()
    for C in (32, 64, 128):
        assert np.array_equal(ys[16], ys[C]), f"y at C = 16 and at C = {C} differ in {(ys[16] != ys[C]).sum()} pixels"


# ====================================================================================================== random inputs
@pytest.mark.parametrize("shape", RANDOM_SHAPES, ids=dc.sid)
def test_random_inputs_elementwise_against_fp64(shape):
    """Every entry point on randn data with two scales, each output element within its own bound; a second call returns the same bits."""
    N, C, H, W = shape
    rows = dc.rows_of(shape)
    d = dc.case(shape, "random")
    x, w, y, dy = (dev(d[k]) for k in ("x", "w", "y", "dy"))
    b = dev(np.array([d["b"]]))
    f, r = d["fwd"], d["bwd"]
    tag = dc.sid(shape)
    P = N * H * W
    a = run_fwd(x, w, b, shape)
    within(a.np((N, H, W)), f["y"], 0.25 * (9 * C + 2) * U * f["z_abs"] + sigmoid_bound(f["y"]), f"{tag} forward, random class")
    assert torch.equal(a.buf.view(torch.int32), run_fwd(x, w, b, shape).buf.view(torch.int32)), f"{tag}: forward not reproducible"
    dx_bound = (r["dx_terms"][None, :, :, None] + 3) * U * r["dx_abs"]
    dw_bound, db_bound = (P + 2) * U * r["dw_abs"], (P + 2) * U * r["db_abs"]
    outs = []
    if dc.BWD_DATA in rows:
        outs.append(("bwd_data", (run_bwd_data(dy, y, w, shape),), lambda: (run_bwd_data(dy, y, w, shape),)))
    if dc.BWD_WEIGHT in rows:
        outs.append(("bwd_weight", run_bwd_weight(dy, y, x, shape), lambda: run_bwd_weight(dy, y, x, shape)))
    if dc.BWD in rows:
        outs.append(("bwd", run_bwd(dy, y, x, w, shape), lambda: run_bwd(dy, y, x, w, shape)))
    for name, got, again in outs:
        for o in got:
            if o.n == N * H * W * C:
                within(o.np(), r["dx"].ravel(), dx_bound.ravel(), f"{tag} {name} dx")
            elif o.n == 9 * C:
                within(o.np(), r["dw"].ravel(), dw_bound.ravel(), f"{tag} {name} dw")
            else:
                within(o.np()[0], r["db"], db_bound, f"{tag} {name} db")
        for o, o2 in zip(got, again()):
            assert torch.equal(o.buf.view(torch.int32), o2.buf.view(torch.int32)), f"{tag} {name}: not reproducible"


def test_data_gradient_second_pass_random():
    """The 64 MiB row of the data gradient at C = 16 on random data, elementwise against fp64."""
    shape = (1, 16, 1024, 1025)
    d = dc.random_inputs(shape, need_x=False)
    g = np.random.default_rng(5)
    y32 = g.uniform(0.0, 1.0, shape[:1] + shape[2:]).astype(np.float32)
    ref = dc.big_dx(d["w"], y32.astype(np.float64), d["dy"], with_abs=True)
    dx = run_bwd_data(dev(d["dy"]), dev(y32), dev(d["w"]), shape)
    got = dx.body.view(ref["dx"].shape).cpu().double()
    bound = (ref["dx_terms"][None, :, :, None] + 3) * U * ref["dx_abs"]
    ratio = ((got - ref["dx"]).abs() / bound.clamp_min(1e-300)).max().item()
    print(f"{dc.sid(shape)} bwd_data dx: max err / bound = {ratio:.3f}")
    assert ratio <= 1.0
    assert torch.equal(dx.buf.view(torch.int32), run_bwd_data(dev(d["dy"]), dev(y32), dev(d["w"]), shape).buf.view(torch.int32))


def test_direct_forward_second_pass_random():
    """The 64 MiB row of the direct forward at C = 64 on random data, elementwise against fp64."""
    shape = (1, 64, 256, 1025)
    N, C, H, W = shape
    d = dc.random_inputs(shape)
    ref = dc.big_forward(d["x"], d["w"], d["b"])
    y = run_fwd(dev(d["x"]), dev(d["w"]), dev(np.array([d["b"]])), shape).np((N, H, W))
    within(y, ref["y"], 0.25 * (9 * C + 2) * U * ref["z_abs"] + sigmoid_bound(ref["y"]), f"{dc.sid(shape)} forward, random class")


# ====================================================================================================== non-finite values stay local
@pytest.mark.parametrize("C", [16, 64], ids=["tile form", "direct form"])
def test_a_nan_stays_in_its_window(C):
    """One NaN in x makes exactly those y non-finite whose reflected 3x3 window holds the pixel; one NaN in dy makes exactly the dx
    pixels non-finite that this output read (fold included), in all their channels, by both routes.  Everything else keeps its bits."""
    shape = (2, C, 5, 6)
    N, _, H, W = shape
    d = dc.case((2, C, 4, 5), "exact")                       # weights only: all non-zero
    g = np.random.default_rng(C)
    xa = g.integers(-3, 5, (N, H, W, C)) * 0.25
    ya, dya = g.integers(1, 4, (N, H, W)) * 0.25, g.integers(1, 4, (N, H, W)).astype(np.float64)
    w = dev(d["w"])
    clean_y = run_fwd(dev(xa), w, None, shape).np((N, H, W))
    clean = {"bwd_data": run_bwd_data(dev(dya), dev(ya), w, shape).np((N, H, W, C)),
             "bwd": run_bwd(dev(dya), dev(ya), dev(xa), w, shape)[0].np((N, H, W, C))}
    for n, h0, w0 in ((0, 0, 0), (1, 1, 1), (0, 4, 5), (1, 3, 4), (0, 2, 3), (1, 0, 4)):
        xn = xa.copy()
        xn[n, h0, w0, C // 2 + 1] = np.nan
        y = run_fwd(dev(xn), w, None, shape).np((N, H, W))
        want = np.zeros((N, H, W), dtype=bool)
        for h in range(H):
            for q in range(W):
                want[n, h, q] = (h0, w0) in dc.window_pixels(H, W, h, q)
        assert np.array_equal(~np.isfinite(y), want), f"NaN in x at {(n, h0, w0)}: non-finite y at {np.argwhere(~np.isfinite(y)).tolist()}"
        assert np.array_equal(y[~want], clean_y[~want])
        dyn = dya.copy()
        dyn[n, h0, w0] = np.nan
        want = np.zeros((N, H, W), dtype=bool)
        for h, q in dc.window_pixels(H, W, h0, w0):
            want[n, h, q] = True
        for name in ("bwd_data", "bwd"):
            dx = (run_bwd_data(dev(dyn), dev(ya), w, shape) if name == "bwd_data" else run_bwd(dev(dyn), dev(ya), dev(xa), w, shape)[0]).np((N, H, W, C))
            bad = ~np.isfinite(dx)
            assert np.array_equal(bad, np.broadcast_to(want[..., None], bad.shape)), f"NaN in dy at {(n, h0, w0)}, {name}: wrong set of non-finite dx"
            assert np.array_equal(dx[~want], clean[name][~want])


# ====================================================================================================== empty and refused calls
def test_empty_batch_touches_nothing():
    C = 32
    t = torch.zeros(64, device="cuda")
    outs = [Out(16) for _ in range(6)]
    ws = workspace(C)
    ok(lib.pd_disphead_fwd(p(t), p(t), p(t), p(outs[0]), 0, 2, 2, C, stream_ptr()), "fwd")
    ok(lib.pd_disphead_bwd_data(p(t), p(t), p(t), p(outs[1]), 0, 2, 2, C, stream_ptr()), "bwd_data")
    ok(lib.pd_disphead_bwd_weight(p(t), p(t), p(t), p(outs[2]), p(outs[3]), p(ws), ws.numel(), 0, 2, 2, C, 0, stream_ptr()), "bwd_weight")
    ok(lib.pd_disphead_bwd(p(t), p(t), p(t), p(t), None, 0, p(outs[4]), p(outs[2]), p(outs[5]), p(ws), ws.numel(), 0, 2, 2, C, 0, stream_ptr()), "bwd")
    torch.cuda.synchronize()
    for o in outs:
        o.untouched("N == 0")
    assert bool((ws == 255).all())


def test_refused_calls():
    """add / elu without dx, an x that is 4 bytes off its alignment, a workspace one byte short: -22 with a message, nothing written."""
    C = 16
    t = torch.zeros(4 * C + 4, device="cuda")
    off = ctypes.c_void_p(t.data_ptr() + 4)
    dx, dw, db, y = Out(4 * C), Out(9 * C), Out(1), Out(4)
    ws = workspace(C)
    n = ws.numel()
    err = lib.pd_last_error
    st = stream_ptr()
    assert lib.pd_disphead_bwd(p(t), p(t), p(t), p(t), p(t), 0, None, p(dw), p(db), p(ws), n, 1, 2, 2, C, 0, st) == -22 and b"dx, which is NULL" in err()
    assert lib.pd_disphead_bwd(p(t), p(t), p(t), p(t), None, 1, None, p(dw), p(db), p(ws), n, 1, 2, 2, C, 0, st) == -22 and b"dx, which is NULL" in err()
    assert lib.pd_disphead_fwd(off, p(t), p(t), p(y), 1, 2, 2, C, st) == -22 and b"16-byte aligned" in err()
    assert lib.pd_disphead_bwd_weight(p(t), p(t), off, p(dw), p(db), p(ws), n, 1, 2, 2, C, 0, st) == -22 and b"16-byte aligned" in err()
    assert lib.pd_disphead_bwd(p(t), p(t), off, p(t), None, 0, p(dx), p(dw), p(db), p(ws), n, 1, 2, 2, C, 0, st) == -22 and b"16-byte aligned" in err()
    assert lib.pd_disphead_bwd_weight(p(t), p(t), p(t), p(dw), p(db), p(ws), n - 1, 1, 2, 2, C, 0, st) == -22 and b"workspace too small" in err()
    assert lib.pd_disphead_bwd(p(t), p(t), p(t), p(t), None, 0, p(dx), p(dw), p(db), p(ws), n - 1, 1, 2, 2, C, 0, st) == -22 and b"workspace too small" in err()
    torch.cuda.synchronize()
    for o in (dx, dw, db, y):
        o.untouched("refused call")
    assert bool((ws == 255).all())
