#!/usr/bin/env python3
"""Two checkouts of the Python layer over ONE libpolardepth.so: do they issue the same library calls and compute the same bits?

    python tools/conv_nodes_ab.py ab PARENT_ROOT BRANCH_ROOT [--lib SO] [--reps 2] [--save DIR]
    python tools/conv_nodes_ab.py dumps DIR_A DIR_B          # two `bench.py --dump-outputs` directories, array by array

`ab` runs every scenario below with the package of each root in turn (parent, branch, parent, branch, ...), each pass in a fresh
child process whose library is --lib (default: BRANCH_ROOT's own build, through PD_LIB), and prints per scenario the number of
library calls, the sha256 of their ordered trace and the sha256 of every output, input gradient and parameter gradient.  A
trace entry is the function name, every integer and float argument, whether each pointer argument is NULL (element by element
for host arrays) and the stream the call was made on: main, wgrad (functional.wgrad_stream) or the n-th other stream in order of
first use.  The trace comes from a recording object placed over polardepth._lib.lib's handle in the child only.

Scenarios: the case grid of tests/test_conv_nodes_gpu.py (through its `run`), and one seeded forward + backward of the default
trainer, the attention variant, the pose-network step (2 x 64 x 96, as tests/test_step*_gpu.py), a DPT fusion block
(manydepth/dpt/blocks.py, as tests/test_modules_gpu.py) and the decoder with uncertainty heads.

Differences between the parent's and the branch's trace are listed and classified; the exit status is 1 if a hash differs or a
difference is of no permitted kind:
  fold    pd_reflect_fold(...) became pd_reflect_fold_pad(..., 1): the same launch (csrc/elementwise.hip)
  stride1 the channel stride told for a ONE-channel operand (it multiplies channel index 0 only): a one-channel gradient that
          as_nhwc copied, or whose activation gradient is laid out like dy where it used to be laid out like y
"""
import argparse
import hashlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
PKG_DIR = "supervised-depth-estimation-from-polarized-images_amd"
# function -> (index of the operand's channel count, index of its channel stride)
CHANNEL_STRIDE_ARGS = {"pd_conv2d": (9, 13), "pd_conv2d_add": (8, 12), "pd_conv2d_rect": (6, 10)}


# ------------------------------------------------------------------ child: one pass over the scenarios
class Recorder:
    """Stands in for the ctypes handle of polardepth._lib.lib: records every call of a function of _lib.SIGNATURES."""

    def __init__(self, handle, signatures):
        self.handle, self.signatures = handle, signatures
        self.trace, self.streams = [], []

    def _stream(self):
        import torch
        from polardepth import functional as PF
        cur = torch.cuda.current_stream()
        if cur == torch.cuda.default_stream():
            return "main"
        if any(cur == s for s in PF._WGRAD_STREAMS.values()):
            return "wgrad"
        if all(cur != s for s in self.streams):
            self.streams.append(cur)
        return f"other{[cur == s for s in self.streams].index(True)}"

    @staticmethod
    def _arg(a, ctype):
        import ctypes
        if ctype in (ctypes.c_float, ctypes.c_double):
            return float(a)
        if isinstance(a, ctypes.Array):                     # host arrays: ints by value, pointers by NULL-ness
            return [int(v) if isinstance(v, int) and a._type_ is not ctypes.c_void_p else int(bool(v)) for v in a]
        if ctype in (ctypes.c_void_p, ctypes.c_char_p) or issubclass(ctype, ctypes._Pointer):
            return "null" if (a is None or (hasattr(a, "value") and not a.value) or a == 0) else "ptr"
        return int(a)

    def __getattr__(self, name):
        fn = getattr(self.handle, name)
        sig = self.signatures.get(name)
        if sig is None or name == "pd_last_error":
            return fn

        def call(*args):
            self.trace.append([name, [self._arg(a, t) for a, t in zip(args, sig[1])], self._stream()])
            return fn(*args)
        return call


def _sha(t):
    import torch
    if not torch.is_tensor(t):
        return "none"
    return hashlib.sha256(t.detach().float().cpu().contiguous().numpy().tobytes()).hexdigest()[:16]


def _trainer_opts(tmp, posenet):
    from manydepth.options import MonodepthOptions
    only = [] if posenet else ["--depth_supervision_only", "True"]
    opts = MonodepthOptions().parse([
        "--png", "--batch_size", "2", "--height", "64", "--width", "96", "--dataset", "HAMMER", "--split", "HAMMER",
        "--eval_split", "HAMMER_unseen", "--min_depth", "0.1", "--max_depth", "2.0", *only, "--depth_supervision", "True",
        "--normals_loss_weight", "0.35", "--augment_xolp", "--augment_normals", "--log_dir", tmp, "--data_path", "synthetic",
        "--data_path_val", "synthetic", "--num_workers", "0", "--weights_init", "scratch", "--learning_rate", "1e-4",
        *(["--dropout_rate", "0.0"] if posenet else [])])
    if posenet:
        opts.pose_input, opts.pose_network = False, True
    return opts


def _trainer_step(attention=False, posenet=False):
    import torch
    from manydepth.trainer import Trainer
    from polardepth import functional as PF, synthetic
    torch.manual_seed(0)
    opts = _trainer_opts(tempfile.mkdtemp(), posenet)
    opts.joint_attention = attention
    tr = Trainer(opts)
    tr.set_train()
    batch = next(iter(tr.train_loader)) if posenet else synthetic.make_batch(2, 64, 96, frame_w=92, device="cuda", seed=5)
    PF.DropoutState.manual_seed(77)
    tr.model_optimizer.zero_grad()
    torch.manual_seed(77)
    outputs, losses, _ = tr.process_batch(dict(batch), is_train=True)
    losses["loss"].backward()
    PF.sync_wgrad_stream()
    torch.cuda.synchronize()
    out = {"loss": losses["loss"], "param_grads": tr.model_optimizer.store.grad}
    out.update({f"disp{s}": outputs[("disp", s)] for s in opts.scales})
    return out


def _module_step(module, args, leaves, seed):
    """Forward of `module(*args)`, backward of sum(output * noise) over all its outputs; `leaves`: the input tensors."""
    import torch
    from polardepth import functional as PF
    res = module(*args)
    outs = list(res.values()) if isinstance(res, dict) else [res]
    g = torch.Generator().manual_seed(seed)
    sum((o * torch.randn(o.shape, generator=g).cuda()).sum() for o in outs).backward()
    PF.sync_wgrad_stream()
    torch.cuda.synchronize()
    out = {f"out{i}": o for i, o in enumerate(outs)}
    out.update({f"dx{i}": x.grad for i, x in enumerate(leaves)})
    out.update({"d_" + k: p.grad for k, p in module.named_parameters()})
    return out


def _dpt_block():
    import torch
    from manydepth.dpt import blocks
    torch.manual_seed(3)
    blk = blocks.FeatureFusionBlock_custom(64, torch.nn.ReLU(False), deconv=False, bn=False, expand=False, align_corners=True)
    xs = [torch.randn(2, 64, 8, 12).cuda().requires_grad_(True) for _ in range(2)]
    return _module_step(blk.cuda(), xs, xs, 31)


def _uncertainty_decoder():
    import numpy as np
    import torch
    from manydepth import networks
    torch.manual_seed(4)
    dd = networks.DepthDecoder(np.array([64, 64, 128, 256, 512]), range(4), uncertainty=True).cuda()
    feats = [torch.randn(2, c, 32 >> i, 48 >> i).cuda().requires_grad_(True) for i, c in enumerate((64, 64, 128, 256, 512))]
    return _module_step(dd, [feats], feats, 32)


def _grid_case(name):
    import test_conv_nodes_gpu as T
    from polardepth import functional as PF
    if T.CASES[name][10] == "fold_off":
        PF.USE_REFLECT_BORDER = False
    try:
        y, dx, dw, db, _, _ = T.run(name)
    finally:
        PF.USE_REFLECT_BORDER = True
    return {"y": y, "dx": dx, "dw": dw, "db": db}


def child(root, out_path):
    sys.path[:0] = [root, os.path.join(root, PKG_DIR), os.path.join(os.path.dirname(HERE), "tests")]
    import polardepth._lib as L
    rec = Recorder(L.lib._load(), L.SIGNATURES)
    L.lib._h = rec
    import test_conv_nodes_gpu as T
    scenarios = [("grid/" + n, lambda n=n: _grid_case(n)) for n in T.CASES]
    scenarios += [("default_trainer", _trainer_step), ("attention_variant", lambda: _trainer_step(attention=True)),
                  ("pose_network_step", lambda: _trainer_step(posenet=True)), ("dpt_fusion_block", _dpt_block),
                  ("uncertainty_decoder", _uncertainty_decoder)]
    result = {}
    for name, fn in scenarios:
        rec.trace, rec.streams = [], []
        tensors = fn()
        result[name] = {"trace": rec.trace, "hashes": {k: _sha(v) for k, v in tensors.items()}}
    with open(out_path, "w") as f:
        json.dump(result, f)


# ------------------------------------------------------------------ parent process: run, compare, report
def _digest(obj):
    return hashlib.sha256(json.dumps(obj, sort_keys=True).encode()).hexdigest()[:16]


def classify(p, b):
    """'' if the two trace entries are equal, else the kind of their difference."""
    if p == b:
        return ""
    (pn, pa, ps), (bn, ba, bs) = p, b
    if ps == bs and pn == "pd_reflect_fold" and bn == "pd_reflect_fold_pad" and ba == pa[:6] + [1] + pa[6:]:
        return "fold"
    idx = CHANNEL_STRIDE_ARGS.get(pn)
    if ps == bs and pn == bn and idx and len(pa) == len(ba) and pa[idx[0]] == ba[idx[0]] == 1 \
            and all(x == y for i, (x, y) in enumerate(zip(pa, ba)) if i != idx[1]):
        return "stride1"
    return "UNEXPECTED"


def ab(args):
    lib = os.path.abspath(args.lib or os.path.join(args.branch, PKG_DIR, "polardepth", "libpolardepth.so"))
    tmp = args.save or tempfile.mkdtemp()
    os.makedirs(tmp, exist_ok=True)
    runs = {"parent": [], "branch": []}
    for rep in range(args.reps):
        for side, root in (("parent", args.parent), ("branch", args.branch)):
            out = os.path.join(tmp, f"{side}_{rep}.json")
            env = dict(os.environ, PD_LIB=lib)
            subprocess.run([sys.executable, os.path.abspath(__file__), "child", os.path.abspath(root), out], check=True, env=env,
                           timeout=args.child_timeout)
            with open(out) as f:
                res = json.load(f)
            runs[side].append(res)
            print(f"# run {rep + 1} {side}: scenario, library calls, sha256 of the trace, sha256 over all output hashes")
            for name, r in res.items():
                print(f"{name} {len(r['trace'])} {_digest(r['trace'])} {_digest(r['hashes'])}")
    bad = False
    print("# run-to-run: traces and hashes of the repetitions of each side")
    for side, rs in runs.items():
        same = all(r == rs[0] for r in rs[1:])
        bad |= not same
        print(f"{side}: {len(rs)} runs {'identical' if same else 'DIFFER'}")
    print("# parent against branch (run 1 of each): outputs and gradients, then the differing trace entries")
    P, B = runs["parent"][0], runs["branch"][0]
    for name in P:
        hp, hb = P[name]["hashes"], B[name]["hashes"]
        differ = sorted(k for k in set(hp) | set(hb) if hp.get(k) != hb.get(k))
        tp, tb = P[name]["trace"], B[name]["trace"]
        kinds = [classify(p, b) for p, b in zip(tp, tb)] if len(tp) == len(tb) else ["UNEXPECTED"]
        count = {k: kinds.count(k) for k in ("fold", "stride1", "UNEXPECTED") if k in kinds}
        bad |= bool(differ) or "UNEXPECTED" in count
        print(f"{name}: {len(hp)} tensors, {'all equal' if not differ else 'DIFFERENT: ' + ', '.join(differ)}; "
              f"{len(tp)} / {len(tb)} calls, {'trace identical' if not count else 'differences: ' + json.dumps(count)}")
        shown = set()
        for p, b, k in zip(tp, tb, kinds):
            if k and (k == "UNEXPECTED" or (p[0], k) not in shown):      # one example per function of the permitted kinds
                shown.add((p[0], k))
                print(f"    [{k}] parent {p[0]}{tuple(p[1])}@{p[2]}\n    {' ' * len(k)}   branch {b[0]}{tuple(b[1])}@{b[2]}")
        if len(tp) != len(tb):
            i = next((i for i, (p, b) in enumerate(zip(tp, tb)) if p != b), min(len(tp), len(tb)))
            print(f"    first divergence at call {i}: parent {tp[i:i + 1]} branch {tb[i:i + 1]}")
    print("RESULT:", "FAILED" if bad else "all hashes equal; every trace difference is of a permitted kind")
    return int(bad)


def dumps(args):
    import numpy as np
    a, b = (sorted(f for f in os.listdir(d) if f.endswith(".npy")) for d in (args.a, args.b))
    bad = a != b
    for f in a if not bad else ():
        x, y = np.load(os.path.join(args.a, f)), np.load(os.path.join(args.b, f))
        same = x.shape == y.shape and x.dtype == y.dtype and x.tobytes() == y.tobytes()
        bad |= not same
        if not same:
            print("DIFFERENT:", f)
    print(f"dumped arrays: {len(a)} / {len(b)} files,", "NOT bit-identical" if bad else "every array bit-identical")
    return int(bad)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    sub = ap.add_subparsers(dest="cmd", required=True)
    p = sub.add_parser("ab")
    p.add_argument("parent"); p.add_argument("branch")
    p.add_argument("--lib", default=None); p.add_argument("--reps", type=int, default=2); p.add_argument("--save", default=None)
    p.add_argument("--child-timeout", type=int, default=240)
    p = sub.add_parser("dumps")
    p.add_argument("a"); p.add_argument("b")
    p = sub.add_parser("child")
    p.add_argument("root"); p.add_argument("out")
    args = ap.parse_args()
    if args.cmd == "child":
        return child(args.root, args.out)
    return ab(args) if args.cmd == "ab" else dumps(args)


if __name__ == "__main__":
    sys.exit(main())
