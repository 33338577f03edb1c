"""BoT-SORT with `gmc_method: orb` / `sift` / `ecc` through the frame-sharded run (geotrax_amd.extract.track_with_model_sharded):
two gloo ranks on the one GPU, three runs per rank (a priming frame mid-clip for orb / sift, the clip's first frame as the
template of the rank that does not hold it for ecc), a frame without detections -- against the single-process run, byte for
byte, tables and per-frame warps. And the unsharded pipelined engine with orb against the frame-at-a-time loop.

Run as a script (`python -m torch.distributed.run ... tests/test_sharded_gmc_gpu.py clip cfg out`) this file is one rank."""
import argparse
import logging
import os
import subprocess
import sys
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
pytestmark = pytest.mark.gpu
logger = logging.getLogger("test_sharded_gmc")
N_FRAMES, FLAT_AT = 12, 5


def _setup(clip, cfg_path):
    from geotrax_amd import extract as ex
    from geotrax_amd.config_utils import load_config_all

    args = argparse.Namespace(source=str(clip), cfg=cfg_path, output_folder=None, log_path=None, verbose=False, model=None,
                              class_names=None, conf=None, classes=None, cut_frame_left=None, cut_frame_right=None, interpolate=None)
    model = ex.load_detector(args, logger)
    config = load_config_all(args, logger, model_names=model.names)
    args.cut_frame_left, args.cut_frame_right = 0, None
    return model, config


def _record_warps(model, warps):
    """Every warp the tracker is given, in clip order: update(gmc=) in the single-process run, the records' GMC block in rank 0's replay."""
    from geotrax_amd import distributed as D

    make = model._make_tracker

    def make_tracker(params):
        t = make(params)
        update, replay = t.update, t.replay

        def rec_update(*a, gmc=None, **kw):
            warps.append(None if gmc is None else np.array(gmc, np.float64))
            return update(*a, gmc=gmc, **kw)

        def rec_replay(recs, max_det, with_gmc=False):
            warps.extend(D.unpack_frame_gmc(r) for r in recs)
            return replay(recs, max_det, with_gmc=with_gmc)

        t.update, t.replay = rec_update, rec_replay
        return t

    model._make_tracker = make_tracker


def _rank_main(clip, cfg_path, out):
    from geotrax_amd import distributed as D
    from geotrax_amd import extract as ex

    model, config = _setup(clip, Path(cfg_path))
    warps = []
    _record_warps(model, warps)
    res = ex.track_with_model_sharded(model, config, logger)
    if res is not None:
        np.savez(out, tracks=res[0], transforms=res[1], warps=np.stack(warps))
    D.shutdown_process_group()


def _clip_and_cfg(gtx_ctx, tmp_path, method):
    import yaml
    from geotrax_amd.model import YOLO
    from geotrax_amd.synth import make_scene
    from test_extract_gpu import H, W, _cfg_file, _weights_file

    sc = make_scene(seed=4, h=H, w=W)
    frames = [sc.render(3 * t, 150) for t in range(N_FRAMES)]
    wpath, _ = _weights_file(tmp_path, gtx_ctx, frames[0])
    cfg_path, cfg = _cfg_file(tmp_path, wpath, tracker="botsort", gmc_method=method)
    cfg["stabilo"]["mask_use"] = False                       # shard ranks mask with the raw detections, the single run with the tracker's boxes
    cfg["engine"] = {"shard_run_frames": 2}                  # 6 runs of one batch: three per rank
    if method == "ecc":
        cfg["engine"]["gmc"] = {"warp": "exact", "max_iters": 30}
    cfg_path.write_text(yaml.safe_dump(cfg))
    probe = YOLO(wpath, ctx=gtx_ctx)
    flat = next((c for c in (np.full((H, W, 3), v, np.uint8) for v in (0, 114, 255, 64, 192, 32)) if len(probe.predict(c, **cfg["ultralytics"])[0].boxes) == 0), None)
    if probe.detector is not None:
        probe.detector.close()
    assert flat is not None, "no flat image is empty for the seeded detector"
    frames[FLAT_AT] = flat
    clip = tmp_path / "clip.npy"
    np.save(clip, np.stack(frames))
    return clip, cfg_path


@pytest.mark.parametrize("method,port", [("orb", 29561), ("sift", 29562), ("ecc", 29563)])
def test_two_ranks_equal_the_single_process_run(gtx_ctx, tmp_path, method, port):
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(gtx_ctx, tmp_path, method)
    model, config = _setup(clip, cfg_path)
    warps = []
    _record_warps(model, warps)
    tracks, transforms = ex.track_with_model(model, config, logger)
    assert len(tracks) > 20 and len(warps) == N_FRAMES and FLAT_AT not in set(tracks[:, 0].astype(int))
    assert sum(not np.array_equal(w, np.eye(2, 3)) for w in warps) >= N_FRAMES - 4           # the method did estimate motion
    out = tmp_path / "rank0.npz"
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", GTX_DIST_BACKEND="gloo", OMP_NUM_THREADS="1",
               PYTHONPATH=os.pathsep.join([str(ROOT / "geo-trax_amd"), str(ROOT), str(ROOT / "tests"), os.environ.get("PYTHONPATH", "")]))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", str(port), str(Path(__file__).resolve()), str(clip), str(cfg_path), str(out)]
    p = subprocess.run(cmd, capture_output=True, text=True, timeout=300, cwd=tmp_path, env=env)      # one attempt, its own time limit
    assert p.returncode == 0 and out.exists(), (p.stdout + p.stderr)[-3000:]
    got = np.load(out)
    assert got["tracks"].dtype == tracks.dtype and got["tracks"].tobytes() == tracks.tobytes()
    assert got["transforms"].dtype == transforms.dtype and got["transforms"].tobytes() == transforms.tobytes()
    assert got["warps"].tobytes() == np.stack(warps).tobytes()


def test_pipelined_engine_with_orb_equals_the_blocking_loop(gtx_ctx, tmp_path):
    from geotrax_amd import extract as ex

    clip, cfg_path = _clip_and_cfg(gtx_ctx, tmp_path, "orb")
    model, config = _setup(clip, cfg_path)
    t1, h1 = ex.track_with_model(model, config, logger)
    model, config = _setup(clip, cfg_path)
    config['main'].setdefault('engine', {})['pipelined'] = False
    t2, h2 = ex.track_with_model_blocking(model, config, logger)
    assert len(t1) > 20 and t1.tobytes() == t2.tobytes() and h1.tobytes() == h2.tobytes()


if __name__ == "__main__":
    _rank_main(*sys.argv[1:4])
