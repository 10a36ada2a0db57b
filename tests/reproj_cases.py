"""Test helper: the case table of the reduction over the frames (pd_reproj_combine_fwd), built from fixture G12's own fp32
maps -- shared by the device test (tests/test_reproj_gpu.py) and the CPU oracle's test (tests/test_oracle_reproj.py)."""
import numpy as np

COMBINE_CASES = ["fixture", "no_noise", "no_automask", "avg", "avg_invalid", "item_without_frames", "first_frame_invalid",
                 "tie_between_frames", "tie_with_identity"]


def combine_cases(g12):
    r = [g12["reproj0_f32"].copy(), g12["reproj1_f32"].copy()]
    i = [g12["ident0_f32"], g12["ident1_f32"]]
    tie = [r[0].copy(), r[1].copy()]
    tie[1][:, :, 3:9] = tie[0][:, :, 3:9]                                           # equal maps: frame 0 must win
    tie_id = [i[0].copy(), i[1].copy()]
    tie_id[0][0, 0, :5] = tie_id[1][0, 0, :5] = np.minimum(r[0], r[1])[0, 0, :5]    # reprojection == identity: kept
    return {
        "fixture": dict(reproj=r, identity=i, noise=g12["noise"]),
        "no_noise": dict(reproj=r, identity=i),
        "no_automask": dict(reproj=r),
        "avg": dict(reproj=r, identity=i, noise=g12["noise"], avg=True),
        "avg_invalid": dict(reproj=r, identity=i, valid=np.array([[1, 0], [1, 1]], np.float32), avg=True),
        "item_without_frames": dict(reproj=r, identity=i, noise=g12["noise"], valid=np.array([[0, 0], [1, 1]], np.float32)),
        "first_frame_invalid": dict(reproj=r, identity=i, valid=np.array([[0, 1], [1, 0]], np.float32)),
        "tie_between_frames": dict(reproj=tie),
        "tie_with_identity": dict(reproj=r, identity=tie_id),
    }
