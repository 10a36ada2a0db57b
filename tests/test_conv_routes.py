"""Which kernel a convolution gets is decided once (route_conv / route_wgrad in csrc/conv.hip); launches, host queries and
profiler labels read that decision.  The recorded table of the commit before that refactoring pins it (host logic, no GPU)."""
import numpy as np
import pytest

import conv_routes
from polardepth import _lib, ops


@pytest.fixture(scope="module")
def tables():
    with np.load(conv_routes.FIXTURE) as z:
        want = {k: z[k] for k in z.files}
    return want, conv_routes.record(_lib.lib, ops)


def test_fixture_holds_every_documented_answer(tables):
    """A sweep that degenerated (all zero, one family) could not pin anything: every documented code of every query occurs."""
    want, _ = tables
    assert len(str(want["commit"])) == 40
    assert len(want["fwd_x3"]) == 579150 and len(want["wgrad_x3"]) == 77220
    assert set(np.unique(want["fwd_x3"])) == {0, 1, 2, 3}
    assert set(np.unique(want["fwd_bf16"])) == {0, 3}
    assert set(np.unique(want["fwd_tile_m"])) == {64, 128}
    assert set(np.unique(want["wgrad_x3"])) == {0, 1, 2, 3}
    assert set(np.unique(want["wgrad_bf16"])) == {0, 2, 3}
    for fam in ("conv_igemm_kernel", "conv_igemm_uni_kernel", "conv_igemm_x3_kernel", "conv_halo_x3_kernel", "conv_halo_bf16_kernel"):
        assert any(n.startswith(fam + "<") for n in want["label_names"]), fam
    assert len(np.unique(want["fwd_label"])) == len(want["label_names"])


@pytest.mark.parametrize("key", ["fwd_x3", "fwd_bf16", "fwd_tile_m", "wgrad_x3", "wgrad_bf16", "wgrad_workspace"])
def test_queries_reproduce_the_recorded_table(tables, key):
    want, got = tables
    bad = np.flatnonzero(want[key] != got[key])
    pts = list(conv_routes.wgrad_points() if key.startswith("wgrad") else conv_routes.fwd_points())
    assert bad.size == 0, [(pts[i], int(want[key][i]), int(got[key][i])) for i in bad[:5]]


def test_labels_reproduce_the_recorded_table(tables):
    """Byte for byte -- but for ONE correction: 96 output columns on 128-row tiles run launch_conv<128, 32, 32, 32> (three
    32-wide column tiles), which the recorded Python rule labelled <128,64>.  The label now names the tile that runs."""
    want, got = tables
    want_s, got_s = want["label_names"][want["fwd_label"]], got["label_names"][got["fwd_label"]]
    co = np.array([p[1] for p in conv_routes.fwd_points()])
    fixed = {"conv_igemm_uni_kernel<128,64>": "conv_igemm_uni_kernel<128,32>", "conv_igemm_kernel<128,64,vec>": "conv_igemm_kernel<128,32,vec>"}
    corrected = (co == 96) & (want["fwd_tile_m"] == 128) & np.isin(want_s, list(fixed))
    assert corrected.any()
    want_s = np.where(corrected, np.array([fixed.get(s, s) for s in want["label_names"]])[want["fwd_label"]], want_s)
    bad = np.flatnonzero(want_s != got_s)
    pts = list(conv_routes.fwd_points())
    assert bad.size == 0, [(pts[i], want_s[i], got_s[i]) for i in bad[:5]]
