"""reference manydepth/evaluation_main.py:7-10; PD_EVAL_NORMALS=1 adds the surface-normal report (Evaluation.test_normals),
PD_EVAL_POINTCLOUD=1 the point-cloud report (Evaluation.test_pointcloud)."""
import os

from manydepth.evaluation import Evaluation


def main():
    ev = Evaluation()
    ev.load_mono_model()
    ev.test()
    if os.environ.get("PD_EVAL_NORMALS") == "1":
        ev.test_normals()
    if os.environ.get("PD_EVAL_POINTCLOUD") == "1":
        ev.test_pointcloud()


if __name__ == "__main__":
    main()
