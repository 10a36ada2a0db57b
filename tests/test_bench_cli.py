"""bench.py's command line and its --dump-outputs writer (host logic, no GPU).  bench is imported in a child process:
its import sets an environment default for RCCL that must not leak into the GPU tests of this process."""
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# stand-ins of the real step's shapes (B = 16, 512x640, scales 0-3), dumped twice into two folders
DUMP_SCRIPT = r"""
import json, os, sys, types
import numpy as np, torch
import bench
B, H, W = 16, 512, 640
g = torch.Generator().manual_seed(0)
outs = {}
for s in range(4):
    d = torch.rand(B, 1, H >> s, W >> s, generator=g)
    outs[("disp", s)] = d; outs[("disp", 0, s)] = d
    dep = torch.rand(B, 1, H, W, generator=g)
    outs[("depth", 0, s)] = dep; outs[("mono_depth", 0, s)] = dep
losses = {"loss": torch.tensor(1.25)}
for s in range(4):
    losses[f"loss/{s}"] = torch.tensor(0.5 + s)
params = [torch.nn.Parameter(torch.randn(3000, 1000, generator=g)), torch.nn.Parameter(torch.randn(64, 3, 7, 7, generator=g))]
tr = types.SimpleNamespace(parameters_to_train=params)
for d in sys.argv[1:]:
    bench.dump_outputs(d, tr, {"outputs": outs, "losses": losses})
print(json.dumps({"disp_2": outs[("disp", 2)].numpy().tolist()[0][0][0][:4], "loss_s3": 3.5}))
"""


def _run(args, **kw):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=300, **kw)


def test_bench_help_lists_full_and_dump_outputs():
    r = _run(["bench.py", "--help"])
    assert r.returncode == 0, r.stderr
    assert "--full" in r.stdout and "--dump-outputs DIR" in r.stdout


def test_dump_outputs_names_dtypes_size_and_repeatability(tmp_path):
    import numpy as np
    a, b = tmp_path / "a", tmp_path / "b"
    r = _run(["-c", DUMP_SCRIPT, str(a), str(b)])
    assert r.returncode == 0, r.stderr
    ref = json.loads(r.stdout.strip().splitlines()[-1])
    names = sorted(os.listdir(a))
    assert names == sorted(os.listdir(b))
    want = {"loss", "loss_s0", "loss_s1", "loss_s2", "loss_s3", "params"} | {f"disp_{s}" for s in range(4)} | \
           {f"depth_0_{s}" for s in range(4)}
    assert names == sorted(n + ".npy" for n in want)             # one file per array; aliases written once
    total = 0
    for n in names:
        x, y = np.load(a / n), np.load(b / n)
        assert x.dtype in (np.float32, np.float64), (n, x.dtype)
        assert np.array_equal(x, y), n                            # a fixed sample: the same elements every time
        total += x.nbytes
    assert total <= 64 << 20
    assert np.load(a / "loss_s3.npy").dtype == np.float64 and float(np.load(a / "loss_s3.npy")) == ref["loss_s3"]
    small = np.load(a / "disp_2.npy")                             # 327680 elements: kept whole, in its shape
    assert small.shape == (16, 1, 128, 160) and small[0, 0, 0, :4].tolist() == ref["disp_2"]
    assert np.load(a / "disp_0.npy").shape == (1 << 20,)          # 5.2 M elements: the seeded sample
    assert np.load(a / "params.npy").shape == (1 << 20,)
