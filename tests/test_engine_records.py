"""Host-side pieces the engine, the stabilizer classes and the sharded replay share: the queue bounds, the last-known-transform
rule, the working -> frame pixel step, the stabilizers' common base and the GMC classes' `wants_frames`. No GPU."""
import itertools

import numpy as np
import pytest

GRAY_RING = 16          # GTX_GRAY_RING of include/gtx.h

QUEUE_CASES = [(1, 1, 1), (1, 2, 4), (2, 2, 4), (2, 4, 4), (4, 4, 4),
               (1, 1, 20),      # more stabilizers than the gray ring covers
               (1, 16, 1),      # batches too large for the GMC's result ring
               (2, 7, 4)]       # (2 + 2 + 2) * 7 + 1 = 43 prepared ECC frames


@pytest.mark.parametrize("gmc", ["none", "gray", "frames"])
@pytest.mark.parametrize("n_dets,B,n_stabs", QUEUE_CASES)
def test_queue_depths(n_dets, B, n_stabs, gmc):
    from geotrax_amd import _lib
    from geotrax_amd.engine import queue_depths

    assert _lib.GRAY_RING == GRAY_RING
    # the three bounds, written out: frames between stage 1 and the stabilizers' collect against the gray ring, the batches ahead
    # of the tracker stage against the GMC's 64-deep result ring, the frames prepared for ECC against its 32-deep ring
    broken = []
    if (2 + 1) * B + 2 * B * n_dets + n_stabs + 1 > (16 - 2) * n_dets * B:
        broken.append("gray ring")
    if gmc != "none" and (2 + 2) * B > 63:
        broken.append("64-deep result ring")
    if gmc == "frames" and (n_dets + 2 + 2) * B + 1 > 31:
        broken.append("32-deep frame ring")
    args = (n_dets, B, n_stabs, gmc != "none", gmc == "frames")
    if broken:
        with pytest.raises(AssertionError, match=broken[0]):
            queue_depths(*args)
    else:
        assert queue_depths(*args) == (2, 2 * B * n_dets)


def test_queue_depths_every_bound_is_reached():
    """The cases above trip each of the three asserts at least once, and the issue's own example trips the ECC one."""
    from geotrax_amd.engine import queue_depths

    with pytest.raises(AssertionError, match="outlive the detector's gray ring"):
        queue_depths(1, 1, 20, False, False)
    with pytest.raises(AssertionError, match="outrun the GMC's 64-deep result ring"):
        queue_depths(1, 16, 1, True, False)
    with pytest.raises(AssertionError, match="outrun the ECC GMC's 32-deep frame ring"):
        queue_depths(4, 4, 4, True, True)                       # (4 + 2 + 2) * 4 + 1 = 33 > 31
    assert queue_depths(4, 4, 4, True, False) == (2, 32)        # the same engine with a GMC that reads gray images


@pytest.mark.parametrize("copy", [True, False])
def test_last_known(copy):
    from geotrax_amd.geometry import LastKnown

    H1, H2 = np.arange(9.0).reshape(3, 3) + 1, np.eye(3) * 2
    want = [(None, False), (H1, False), (H1, True), (H2, False), (H2, True)]
    last = LastKnown(copy=copy)
    for H, (w, fell_back) in zip([None, H1, None, H2, None], want):
        got, fb = last.update(None if H is None else H.copy())
        assert fb is fell_back
        assert (got is None) if w is None else got.tobytes() == w.tobytes()
    last.reset()
    assert last.update(None) == (None, False)


def test_last_known_hands_out_copies():
    """The engine's use (copy=True): whatever a caller does to a matrix it was given, the next frame gets the transform as it was."""
    from geotrax_amd.geometry import LastKnown

    H1 = np.arange(9.0).reshape(3, 3) + 1
    last, mine = LastKnown(), H1.copy()
    got, _ = last.update(mine)
    got[:] = -1                                                 # the caller's own array, returned as it came
    back, fb = last.update(None)
    assert fb and back.tobytes() == H1.tobytes()
    back[:] = -2
    again, fb = last.update(None)
    assert fb and again.tobytes() == H1.tobytes()


@pytest.mark.parametrize("ratio", [0.5, 0.75, 1.0])
def test_work_to_frame(ratio):
    from geotrax_amd.geometry import work_to_frame

    Hw = np.array([[1.01, -0.02, 3.5], [0.015, 0.99, -2.25], [1e-5, -2e-5, 1.3]])
    D = np.diag([ratio, ratio, 1.0])
    Hf = np.linalg.inv(D) @ Hw @ D
    assert work_to_frame(Hw, ratio).tobytes() == (Hf / Hf[2, 2]).tobytes()


def test_stabilized_boxes_without_a_transform_is_a_copy():
    from geotrax_amd.geometry import stabilized_boxes, warp_boxes

    xywh = np.array([[10, 20, 4, 6], [30.5, 40.5, 8, 2]], np.float32)
    out = stabilized_boxes(None, xywh)
    assert out is not xywh and out.tobytes() == xywh.tobytes()
    H = np.array([[1.0, 0.0, 5.0], [0.0, 1.0, -3.0], [0.0, 0.0, 1.0]])
    assert stabilized_boxes(H, xywh).tobytes() == warp_boxes(H, xywh).tobytes()


def test_xyxy_to_xywh_has_one_home():
    from geotrax_amd import distributed, engine, geometry

    assert engine.xyxy_to_xywh is geometry.xyxy_to_xywh is distributed.xyxy_to_xywh and not hasattr(distributed.Replayer, "_xywh")
    assert geometry.xyxy_to_xywh(np.zeros((0, 4), np.float32)) is None
    got = geometry.xyxy_to_xywh(np.array([[1, 2, 4, 10]], np.float64))
    assert got.dtype == np.float32 and got.tolist() == [[2.5, 6.0, 3.0, 8.0]]


SHARED = ["close", "__del__", "_boxes", "_finish", "get_cur_trans_matrix", "registered", "transform_cur_boxes", "get_cur_num_keypoints",
          "get_cur_num_matches", "get_cur_inliers_count"]


def test_the_stabilizer_classes_share_one_base():
    from geotrax_amd.sift_stabilizer import SiftStabilizer
    from geotrax_amd.stabilizer import Stabilizer
    from geotrax_amd.stabilizer_base import _StabilizerBase

    for cls, name in itertools.product((Stabilizer, SiftStabilizer), SHARED):
        assert issubclass(cls, _StabilizerBase) and name in vars(_StabilizerBase)
        assert name not in vars(cls), (cls.__name__, name)
        assert getattr(cls, name) is getattr(_StabilizerBase, name)
    assert Stabilizer._destroy == "gtx_stabilizer_destroy" and SiftStabilizer._destroy == "gtx_sift_stab_destroy"


def test_the_base_keeps_the_last_known_transform():
    """stabilo's rule through the shared _finish: a frame without a transform of its own reports the last known one, `registered`
    and raw=True say so, a new reference forgets it."""
    from geotrax_amd.stabilizer import Stabilizer

    st = Stabilizer(None, ctx=object(), min_good_match_count_warning=0, min_inliers_match_count_warning=0)   # no frame size yet: no library object
    H1 = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, 3.0], [0.0, 0.0, 1.0]])
    boxes = np.array([[10, 10, 4, 4]], np.float32)
    st._finish(None, boxes)
    assert st.get_cur_trans_matrix() is None and not st.registered and st.transform_cur_boxes().tobytes() == boxes.tobytes()
    st._finish(H1.copy(), boxes)
    assert st.registered and st.get_cur_trans_matrix().tobytes() == H1.tobytes()
    st._finish(None, None)
    assert not st.registered and st.get_cur_trans_matrix(raw=True) is None and st.get_cur_trans_matrix().tobytes() == H1.tobytes()
    assert st.transform_cur_boxes().shape == (0, 4)
    st._new_reference()
    assert st.get_cur_trans_matrix() is None


def test_wants_frames_is_a_class_attribute():
    from geotrax_amd.gmc import GMC, EccGMC, FeatureGMC

    assert vars(GMC)["wants_frames"] is False and vars(FeatureGMC)["wants_frames"] is False and vars(EccGMC)["wants_frames"] is True
