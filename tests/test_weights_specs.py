"""The spec lists weights.py builds from its yaml tables, pinned per family and scale. No GPU needed.

The digests were taken from the hand-written spec functions the tables replaced (commit 0c4929d), not from the table walk: a
row, a width rule or a name that drifts changes one of them."""
import hashlib
import itertools
import json

# sha256 (first 16 hex digits) of json.dumps([[name, list(shape), has_act], ...]) at nc = 4 (detectors) / 1000 (cls)
DIGESTS = {
    "yolov8_layer_specs": {"n": "68dff336a0b7b34d", "s": "ce3d900d53e0c3b4", "m": "aaf7ac0e9471a28f", "l": "3b21574d96f427b9", "x": "35fd7baff19629a4"},
    "yolov8_p2_layer_specs": {"n": "384c88b88a3540bb", "s": "f987041d2c1562ab", "m": "e1c5c11fe9f70113", "l": "8b2b3e1b4f3bb991", "x": "cbb1fd4a2791535e"},
    "yolo11_layer_specs": {"n": "3f99485c8a7e4953", "s": "c0aa3aa9c3278a7f", "m": "eb7d8a173ea027f2", "l": "c1dd562a35e02519", "x": "cef924e08a0b9ce4"},
    "yolov8_cls_layer_specs": {"n": "1947b963c7f0d159", "s": "4f11c8c13fb4da11", "m": "24d81df373d629ab", "l": "ffa67a63d218257f", "x": "d4f5efa0576c17d4"},
}
COUNTS = {"yolov8_layer_specs": (63, 63, 83, 103, 103), "yolov8_p2_layer_specs": (78, 78, 102, 126, 126),
          "yolo11_layer_specs": (87, 87, 112, 173, 173), "yolov8_cls_layer_specs": (27, 27, 39, 51, 51)}


def test_spec_lists_are_the_pinned_ones():
    from geotrax_amd import weights

    for fn, (k, scale) in itertools.product(DIGESTS, enumerate("nsmlx")):
        nc = 1000 if fn == "yolov8_cls_layer_specs" else 4
        specs = getattr(weights, fn)(scale, nc)
        assert len(specs) == COUNTS[fn][k], (fn, scale, len(specs))
        assert all(type(d) is int for _, s, _ in specs for d in s) and all(type(a) is bool for _, _, a in specs)
        got = hashlib.sha256(json.dumps([[n, list(s), a] for n, s, a in specs]).encode()).hexdigest()[:16]
        assert got == DIGESTS[fn][scale], (fn, scale, got)
