"""k_tile_ranges (csrc/gsr_binning.hip) at the edges of its rounds, against the exact list reference (tests/binning_ref.py).

The kernel scans a gather chunk's per-rank instance counts and the frame's per-tile counts in rounds of 8192 elements, read and
written coalesced and handed to the block scan through a padded LDS array.  Frames: 2048x1040 = 8320 tiles (a full round and a
partial second one) under a few hundred large splats; 256x192 = 192 tiles (a fraction of one round); and 12 000 wide, faint splats on
1280x720, one gather chunk of more than 8192 and at most 16384 Gaussians - the rank scan's second round.  Ranges, lists and quadrant
bits are checked the way tests/test_gpu_binning_paths.py checks its frames: through its run_frame, with this file's scenes.
"""
import pytest

import binning_ref as BR
import scene_synth as S
import test_gpu_binning_paths as BP

pytestmark = pytest.mark.gpu


def _frame(name):
    if name == "tiles_8320":
        return S.make_scene(300, 2048, 1040, 1, 311, scale_lo=0.5, scale_hi=2.0), S.make_camera(2048, 1040), None
    if name == "tiles_192":
        return S.make_scene(100, 256, 192, 1, 312, scale_lo=0.5, scale_hi=2.0), S.make_camera(256, 192), None
    if name == "ranks_two_rounds":
        return BP._faint_scene(12000, 1280, 720, 7, 70.0, 0.02), S.make_camera(1280, 720), None
    raise KeyError(name)


@pytest.fixture(scope="module")
def hh(tmp_path_factory):
    return BR.build_harness(str(tmp_path_factory.mktemp("hh_ranges")))


@pytest.mark.parametrize("name", ["tiles_8320", "tiles_192", "ranks_two_rounds"])
def test_ranges_and_lists_match_the_reference(name, hh, monkeypatch):
    monkeypatch.setattr(BP, "_frame", _frame)
    rep = BP.run_frame(name, hh)
    print(BP._summary(rep))
    BP._assert_frame(rep)
    # every chunk of these frames takes the gather with the rank scan fused into k_tile_ranges
    assert rep["launches"]["tile_gather"] >= 1 and rep["n_sort"] == 0, rep["launches"]
    assert "gather-fused" in rep["names"], rep["names"]
    if name == "ranks_two_rounds":
        assert len(rep["cells"]) == 1 and 8192 < rep["cells"][0]["n"] <= 16384, rep["cells"]
