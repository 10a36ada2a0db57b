#!/usr/bin/env python3
"""Generate tests/golden/g16_pose_chain.npz by RUNNING THE REFERENCE's own Trainer.predict_poses on the CPU in float32:

    manydepth/trainer.py   Trainer.predict_poses (both halves: :669-707 and the matching poses :708-746)
    manydepth/layers.py    transformation_from_parameters                                            (imported)

The method body is compiled from the checkout's source file at run time (the module itself needs tensorboard, kornia and
roma to import), as make_golden_student.py does.  It runs only where the reference checkout is available ($PD_REFERENCE);
the output is data only.  Re-run with:

    PD_REFERENCE=<reference checkout> python tests/golden/make_golden_pose_chain.py

The stub object: num_pose_frames = 2, opt.frame_ids = [0, -1, 1], models["pose_encoder"] the identity, and models["pose"] a
stub that returns [N,2,1,3] parameters formed by a FIXED LINEAR MAP from the six channel means of its input (slot 0: "map_w"
[6,6], "map_b" [6]; slot 1: the negated slot 0, which nothing may use) -- so the fixture also records which frames were
paired, in which order.  Two cases: "a" matching_ids = [0, -1, -2, -3], "b" = [0, 1, -1, -2].  N = 4, pictures 3 x 8 x 12
("frame_{f}" [4,3,8,12] float32, f = -3 .. 1); item 2 has an all-zero frame -2, so the reference's zeroing and its
propagation into -3 are in the data.

Per case C and matching id f != 0: "C_means_{f}" [4,6] (the channel means the pose stub saw), "C_aa_{f}" / "C_tr_{f}" [4,3]
(slot 0), "C_rel_{f}" / "C_relinv_{f}" [4,4,4] (inputs[("relative_pose", f)] / ("relative_pose_inv", f)); "C_ids" the
matching ids; "C_dev" the observed max |tests/pose_chain_ref - reference| over the case's relative poses.

The generator asserts the fixture's conditions: an absent frame in mid-chain, every link's angle in (0.05, 1.1] (the range
the bound of tests/test_pose_ref.py assumes), non-zero translations."""
import os
import sys
import types

import numpy as np
import torch

REF = os.environ.get("PD_REFERENCE")
OUT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(OUT))
N, H, W = 4, 8, 12
FRAMES = (-3, -2, -1, 0, 1)
ABSENT = (2, -2)                                  # (item, frame)
CASES = {"a": [0, -1, -2, -3], "b": [0, 1, -1, -2]}
SEED = 16


def frames(rng):
    """One level per (frame, item, channel) plus a little texture: the six channel means of a pair identify it."""
    out = {}
    for f in FRAMES:
        level = rng.uniform(0.15, 0.85, (N, 3, 1, 1))
        out[f] = (level + 0.05 * rng.standard_normal((N, 3, H, W))).astype(np.float32)
    out[ABSENT[1]][ABSENT[0]] = 0.0
    return out


def main():
    if not REF or not os.path.isdir(REF):
        sys.exit("set PD_REFERENCE to the reference checkout")
    sys.path.insert(0, os.path.join(REF, "manydepth"))
    import layers
    from make_golden_student import methods_of
    import pose_chain_ref as C
    ns = {"torch": torch, "transformation_from_parameters": layers.transformation_from_parameters}
    (predict_poses,) = methods_of(os.path.join(REF, "manydepth", "trainer.py"), "Trainer", ["predict_poses"], ns)

    rng = np.random.default_rng(SEED)
    pics = frames(rng)
    map_w = rng.uniform(-0.45, 0.45, (6, 6)).astype(np.float32)
    map_b = np.array([0.21, -0.17, 0.13, 0.05, -0.08, 0.11], np.float32)
    data = {f"frame_{f}": pics[f] for f in FRAMES}
    data["map_w"], data["map_b"] = map_w, map_b
    data["absent"] = np.array(ABSENT, np.int64)

    for case, ids in CASES.items():
        calls = []

        def pose(feats):
            x = feats[0]
            means = x.mean((2, 3))                                             # [N,6]
            o = means @ torch.from_numpy(map_w).T + torch.from_numpy(map_b)
            calls.append((means.numpy().copy(), o.numpy().copy()))
            o = torch.stack([o, -o], 1).view(N, 2, 1, 6)
            return o[..., :3], o[..., 3:]

        stub = types.SimpleNamespace(num_pose_frames=2, opt=types.SimpleNamespace(frame_ids=[0, -1, 1]), matching_ids=list(ids),
                                     models={"pose_encoder": lambda x: x, "pose": pose})
        inputs = {("color_aug", f, 0): torch.from_numpy(pics[f]) for f in FRAMES}
        predict_poses(stub, inputs)
        calls = calls[2:]                                                      # the first half's two passes come first
        assert len(calls) == len(ids) - 1
        data[f"{case}_ids"] = np.array(ids, np.int64)
        for fi, (means, o) in zip(ids[1:], calls):
            data[f"{case}_means_{fi}"], data[f"{case}_aa_{fi}"], data[f"{case}_tr_{fi}"] = means, o[:, :3].copy(), o[:, 3:].copy()
            data[f"{case}_rel_{fi}"] = inputs[("relative_pose", fi)].numpy().copy()
            data[f"{case}_relinv_{fi}"] = inputs[("relative_pose_inv", fi)].numpy().copy()
            angle = np.linalg.norm(o[:, :3].astype(np.float64), axis=1)
            assert (angle > 0.05).all() and (angle <= 1.1).all(), (case, fi, angle)
            assert (np.linalg.norm(o[:, 3:].astype(np.float64), axis=1) > 1e-2).all(), (case, fi, o[:, 3:])
        # the absent frame sits in mid-chain: zeroed there, zero behind it, and nowhere else
        neg = [f for f in ids if f < 0]
        assert ABSENT[1] in neg[:-1] or case == "b"
        for fi in ids[1:]:
            zero = ~data[f"{case}_rel_{fi}"].reshape(N, 16).any(1)
            assert zero.tolist() == [n == ABSENT[0] and fi <= ABSENT[1] for n in range(N)], (case, fi, zero)
        dev = 0.0
        for s in (-1, 1):
            chain = sorted([f for f in ids if f * s > 0], key=abs)
            if not chain:
                continue
            aa = np.stack([data[f"{case}_aa_{f}"] for f in chain])
            tr = np.stack([data[f"{case}_tr_{f}"] for f in chain])
            present = np.stack([pics[f].reshape(N, -1).sum(1) != 0 for f in chain]).astype(np.float32)
            rel, _ = C.pose_chain(aa, tr, present, None, s)
            for k, f in enumerate(chain):
                dev = max(dev, float(np.abs(rel[k].astype(np.float64) - data[f"{case}_rel_{f}"]).max()))
        data[f"{case}_dev"] = np.float64(dev)
        print(case, ids, "dev", dev)
    path = os.path.join(OUT, "g16_pose_chain.npz")
    np.savez_compressed(path, **data)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
