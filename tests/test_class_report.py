"""polardepth._records.ClassReport, the driver every per-class evaluator of manydepth.evaluation shares, on a hand-made pool
of CPU tensors (K = 3 classes, batches of N = 2): the per-image mean skips the images a class is missing from and is NaN for
a class no image has, ``+=`` pooling equals one call over all images, a class without a pooled pixel stays in the dict but
not in the table, and the lines are those of the format strings ``Evaluation.test_depth`` has always printed with."""
import numpy as np
import pytest
import torch

from polardepth._records import ClassReport, Pool

METRIC_NAMES = ("mean", "n")
NAMES = ["all", "glass", "wall"]


class Stats(Pool):
    """Records n, bad (int64) and sum (fp64), each [N, K]."""

    def __init__(self, n, bad, total, names=NAMES):
        self.n, self.bad, self.sum = torch.tensor(n), torch.tensor(bad), torch.tensor(total, dtype=torch.float64)
        self.names = list(names)

    def _pool_fields(self):
        return self.n, self.bad, self.sum

    def metrics(self):
        return torch.stack([self.sum / self.n, self.n.double()], -1)

    def pooled(self):
        n, _, s = self._totals()
        return torch.stack([s / n, n.double()], -1)

    def pooled_bad(self):
        return self._totals()[1]


# image:        0            1            2            3           "wall" is in no image, "glass" in images 0 and 3 only
N_PIX = [[4, 2, 0], [4, 0, 0], [2, 0, 0], [8, 4, 0]]
BAD = [[1, 0, 0], [0, 0, 0], [0, 2, 0], [0, 0, 0]]
SUM = [[2.0, 1.0, 0.0], [6.0, 0.0, 0.0], [5.0, 0.0, 0.0], [2.0, 3.0, 0.0]]

TABLE = ("depth (unscaled)      mean         n \n"             # every figure is followed by one blank
         "     all per-image &   1.1875 &   4.5000 \n"
         "     all pooled    &   0.8333 &  18.0000  bad 1\n"
         "   glass per-image &   0.6250 &   3.0000 \n"
         "   glass pooled    &   0.6667 &   6.0000  bad 2\n")


def report(batches):
    rep = ClassReport(METRIC_NAMES)
    for lo, hi in batches:
        st = Stats(N_PIX[lo:hi], BAD[lo:hi], SUM[lo:hi])
        rep.add(st, st.metrics(), st.n > 0)
    return rep, rep.finish("depth (unscaled)")


def test_report_of_two_batches(capsys):
    rep, res = report([(0, 2), (2, 4)])
    assert capsys.readouterr().out == TABLE                  # "wall" has no pooled pixel: not printed
    assert list(res) == NAMES and all(list(r) == ["per_image", "pooled", "bad"] for r in res.values())
    # the mean over the images that have the class: all four, images 0 and 3, none
    assert np.array_equal(res["all"]["per_image"], [(0.5 + 1.5 + 2.5 + 0.25) / 4, 18 / 4])
    assert np.array_equal(res["glass"]["per_image"], [(0.5 + 0.75) / 2, 6 / 2])
    assert np.isnan(res["wall"]["per_image"]).all()
    assert np.array_equal(res["all"]["pooled"], [15.0 / 18, 18.0]) and np.array_equal(res["glass"]["pooled"], [4.0 / 6, 6.0])
    assert np.isnan(res["wall"]["pooled"][0]) and res["wall"]["pooled"][1] == 0
    assert [res[n]["bad"] for n in NAMES] == [1, 2, 0] and all(type(res[n]["bad"]) is int for n in NAMES)
    assert rep.per_image.shape == rep.pooled.shape == (3, 2) and rep.per_image.dtype == np.float64


def test_pooling_batches_equals_one_call(capsys):
    _, split = report([(0, 2), (2, 4)])
    _, whole = report([(0, 4)])
    out = capsys.readouterr().out
    assert out == TABLE + TABLE
    for name in NAMES:
        assert split[name]["bad"] == whole[name]["bad"]
        for key in ("per_image", "pooled"):                  # every sum here is exact in binary
            assert np.array_equal(split[name][key], whole[name][key], equal_nan=True), (name, key)


def test_pooled_only_extras_and_empty(capsys):
    rep = ClassReport(METRIC_NAMES, width=11)
    assert rep.finish("nothing") == {} and capsys.readouterr().out == ""
    for lo, hi in ((0, 2), (2, 4)):
        rep.add(Stats(N_PIX[lo:hi], BAD[lo:hi], SUM[lo:hi]))
    fields = lambda pool: {"n": pool._totals()[0], "pair": torch.stack(pool._totals()[1::-1], -1)}      # [K] and [K, 2]
    res = rep.finish("pairs", extras=fields, show_extras=False)
    assert capsys.readouterr().out == ("pairs        mean           n \n"
                                       "     all pooled    &     0.8333 &    18.0000 \n"
                                       "   glass pooled    &     0.6667 &     6.0000 \n")
    assert list(res["wall"]) == ["pooled", "n", "pair"] and res["all"]["n"] == 18 and type(res["all"]["n"]) is int
    assert np.array_equal(res["glass"]["pair"], [2, 6])
    rep.finish("pairs", extras=lambda pool: {"bad": pool.pooled_bad(), "n": pool._totals()[0]})      # shown, in their order
    assert capsys.readouterr().out.splitlines()[1:] == ["     all pooled    &     0.8333 &    18.0000  bad 1 n 18",
                                                        "   glass pooled    &     0.6667 &     6.0000  bad 2 n 6"]


def test_other_classes_do_not_pool():
    rep = ClassReport(METRIC_NAMES)
    rep.add(Stats(N_PIX[:2], BAD[:2], SUM[:2]))
    with pytest.raises(ValueError, match="cannot pool the classes"):
        rep.add(Stats(N_PIX[2:], BAD[2:], SUM[2:], names=["all", "glass", "table"]))
