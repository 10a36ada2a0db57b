"""reference manydepth/evaluation_main.py:7-10; PD_EVAL_NORMALS=1 adds the surface-normal report (Evaluation.test_normals),
PD_EVAL_POINTCLOUD=1 the point-cloud report (Evaluation.test_pointcloud), PD_EVAL_DEPTH=1 the one-pass depth report
(Evaluation.test_depth), median-scaled with PD_EVAL_MEDIAN_SCALING=numpy or torch, PD_EVAL_POSE=1 the pose report of the
pose network (Evaluation.test_pose; needs PD_POSE_NETWORK=1, which makes Evaluation build and load the pose network),
PD_EVAL_CONSISTENCY=1 the multi-view consistency report of the predicted depth (Evaluation.test_consistency),
PD_EVAL_POLAR_NORMALS=1 the polarimetric normals report (Evaluation.test_polar_normals; PD_POL_AOLP_SIGN=-1 for a sensor of
the other AoLP handedness, PD_POLAR_RAY_FRAME=1 to score in the frame of each pixel's viewing ray), PD_EVAL_UNCERTAINTY=1 the
depth-uncertainty report (Evaluation.test_uncertainty; it makes Evaluation build the decoder with its uncertainty heads, as
PD_UNCERTAINTY=1 does, and the weights folder must hold them), PD_POLAR_REFINE=1 (or "lam,iters") the one-pass depth report
of the depth refined with the polarisation normals (Evaluation.test_depth(source="refined"); Evaluation reads the variable)."""
import os

from manydepth.evaluation import Evaluation


def main():
    ev = Evaluation(uncertainty=True) if os.environ.get("PD_EVAL_UNCERTAINTY") == "1" else Evaluation()
    ev.load_mono_model()
    ev.test()
    if os.environ.get("PD_EVAL_NORMALS") == "1":
        ev.test_normals()
    if os.environ.get("PD_EVAL_POINTCLOUD") == "1":
        ev.test_pointcloud()
    if os.environ.get("PD_EVAL_DEPTH") == "1":
        ev.test_depth(median_scaling=os.environ.get("PD_EVAL_MEDIAN_SCALING") or None)
    if os.environ.get("PD_EVAL_POSE") == "1":
        ev.test_pose()
    if os.environ.get("PD_EVAL_CONSISTENCY") == "1":
        ev.test_consistency()
    if os.environ.get("PD_EVAL_POLAR_NORMALS") == "1":
        ev.test_polar_normals()
    if os.environ.get("PD_EVAL_UNCERTAINTY") == "1":
        ev.test_uncertainty()
    if os.environ.get("PD_POLAR_REFINE") not in (None, "", "0"):
        ev.test_depth(median_scaling=os.environ.get("PD_EVAL_MEDIAN_SCALING") or None, source="refined")


if __name__ == "__main__":
    main()
