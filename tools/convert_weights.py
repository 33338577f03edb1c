#!/usr/bin/env python3
"""Converts an ultralytics YOLOv8 or RT-DETR detect checkpoint (.pt) into the flat .safetensors file +
`<name>.names.yaml` side-car that geotrax_amd.model.YOLO / RTDETR load.

Run this once on a machine where `ultralytics` is installed (it is not part of this build):

    python tools/convert_weights.py geotrax_hbb_yolov8s_1920_v1.pt [out.safetensors]

Conv+BN pairs are fused with ultralytics' own `model.fuse()`; tensor names are the fused model's
state_dict keys (`model.0.conv.weight`, `model.0.conv.bias`, ... `model.22.cv3.2.2.bias`).
A YOLOv8-P2 checkpoint (yolov8<scale>-p2.yaml, geo-trax's train.sh `-p`) goes through the same path unchanged: its fused
state_dict ends in `model.28.cv3.3.2.bias` (Detect on four levels), which is how geotrax_amd.weights.is_yolov8_p2 tells it apart.
A YOLO11 detect checkpoint (yolo11<scale>.yaml) goes through unchanged as well: its fused state_dict has `model.10.m.0.attn.qkv.conv.*`
and ends in `model.23.cv3.2.2.bias`; DWConv and the activation-free Convs (qkv, proj, pe, ffn.1) fold their BN like any Conv.

An RT-DETR checkpoint (the reference's `RTDETR` branch, geotrax/extract.py:222-225; rtdetr-l topology) keeps its state_dict names
too (`model.0.stem1.conv.weight` ... `model.28.decoder.layers.5.norm3.bias`); what `fuse()` leaves unfused -- RepConv's two
branches where a version does not fuse them, the decoder's Sequential(Conv2d, BatchNorm2d) input projections -- is folded by
geotrax_amd.weights.load_weights when the file is read. The decoder's head / point / query counts, which no tensor shape carries,
go into the small `rtdetr.meta` tensor [heads, points, queries, AIFI heads].
A YOLOv8-RTDETR checkpoint (yolov8<scale>-rtdetr.yaml, geo-trax's train.sh `-rt`: the YOLOv8 backbone and neck, RTDETRDecoder =
model.22) takes the same branch ("rtdetr" is in its yaml name); with no AIFI its last `rtdetr.meta` entry falls back to 8 and is unused.

A YOLOv10 detect checkpoint (yolov10{n,s}.yaml) is folded here and not by `model.fuse()`, which would drop v10Detect's one-to-many
branches (`model.23.cv2 / cv3`): convert_state_dict() folds every Conv + BN pair, sums each RepVGGDW's 7x7 and zero-padded 3x3 branch
(weights and BN-folded biases) into the single 7x7 of the fused model (`...cv1.2.conv.weight`), keeps cv2 / cv3 next to one2one_cv2 /
one2one_cv3 -- `end2end: false` runs them through NMS -- and writes `detector.meta` = [family 10, one-to-many kept, end-to-end head,
the head's 300].

A YOLO12 detect checkpoint (yolo12{n,s,m,l,x}.yaml: `model.6.m.0.0.attn.qkv.conv.*`, Detect = model.21) goes through the plain branch:
every Conv + BatchNorm pair of its A2C2f blocks (qkv, proj, the depthwise 7x7 pe, the mlp pair, the C3k members) is folded by fold_bn
like any other, and the `model.6.gamma` / `model.8.gamma` vectors of scales l / x are written as they are.

A YOLOv5u detect checkpoint (yolov5{n,s,m,l,x}u.pt, built from yolov5{n,s,m,l,x}.yaml: a 6x6 `model.0.conv`, Detect = model.24 with its
`dfl`) goes through the plain branch too: the 6x6 stem, the C3 blocks' cv1 / cv2 / cv3 and 1x1 + 3x3 Bottlenecks and the neck's 1x1
Convs are Conv + BatchNorm pairs folded by fold_bn like any other. The P6 files (yolov5*6u), an anchor-based export of the original
YOLOv5, YOLOv3u and the -seg / -cls heads are refused by name when the file is loaded (geotrax_amd.weights.check_yolov5u).

A YOLO26 detect checkpoint (yolo26{n,s,m,l,x}.yaml: `model.22.m.0.1.attn.qkv.*`, 4-row `model.23.*cv2.<l>.2`) takes the same branch: every
Conv + BN pair is folded under its own name (model.22's `m.<k>.0.cv1` Bottleneck and `m.<k>.1.attn.*` / `ffn.*` PSABlock convolutions
included; it has no RepVGGDW), cv2 / cv3 stay next to one2one_cv2 / one2one_cv3, and `detector.meta` = [family 26, one-to-many kept,
end-to-end head, the head's 300].

A YOLOv9 detect checkpoint (yolov9{t,s,m,c}.yaml) goes through `model.fuse()` like YOLOv8: RepConv.fuse_convs leaves one 3x3 under
`...cv2.0.m.<k>.cv1.conv.*`, and the fused state_dict ends in `model.22.cv3.2.2.bias`. Where a version leaves a RepConv's two branches
(`...m.<k>.cv1.conv1` / `conv2`) unfused, geotrax_amd.weights.load_weights folds each branch's BN first and then sums the 1x1 into the
3x3's centre tap (fold_bn, then fuse_repconv). yolov9e (two backbones, CBLinear / CBFuse) is refused when the file is loaded.

A YOLOv8-cls or YOLO11-cls checkpoint (the ReID network of `with_reid: true, model: <file>.safetensors` in a tracker yaml) is written the same
way, plus `cls.meta` = [imgsz] from the checkpoint's training arguments (geotrax_amd.weights.cls_imgsz; 224 when absent).
"""
import sys
from pathlib import Path

import yaml


def convert_state_dict(sd: dict) -> dict:
    """An unfused YOLOv10 or YOLO26 state_dict (numpy arrays under ultralytics' names) -> the flat fused tensors the library reads, plus
    `detector.meta` (geotrax_amd.weights.detector_meta). Needs no ultralytics."""
    import numpy as np

    root = Path(__file__).resolve().parent.parent / "geo-trax_amd"
    if str(root) not in sys.path:
        sys.path.insert(0, str(root))
    from geotrax_amd.weights import V10_MAX_DET, detector_family, family_row, fold_bn, fold_repvggdw, yolov10_has_one2many

    t = {k: np.asarray(v, np.float32) for k, v in sd.items() if "dfl" not in k and "num_batches_tracked" not in k}
    t = fold_repvggdw(fold_bn(t))
    fam = detector_family(t)
    if not fam.end2end:
        raise ValueError(f"convert_state_dict folds YOLOv10 and YOLO26 checkpoints; this one is {fam.graph}")
    t["detector.meta"] = np.asarray([family_row(fam.graph).meta, float(yolov10_has_one2many(t)), 1, V10_MAX_DET], np.float32)
    return t


def main():
    from safetensors.torch import save_file
    from ultralytics import YOLO

    src = Path(sys.argv[1])
    dst = Path(sys.argv[2]) if len(sys.argv) > 2 else src.with_suffix(".safetensors")
    yolo = YOLO(str(src))
    if "rtdetr" in str(getattr(yolo.model, "yaml_file", "") or getattr(yolo.model, "yaml", {}).get("yaml_file", "")):
        from ultralytics import RTDETR

        yolo = RTDETR(str(src))                       # what the reference itself does (extract.py:223-225)
    if any(".one2one_cv2." in k for k in yolo.model.state_dict()):   # YOLOv10 / YOLO26: folded here, so that cv2 / cv3 survive
        from safetensors.numpy import save_file as save_np

        sd = convert_state_dict({k: v.detach().float().numpy() for k, v in yolo.model.float().eval().state_dict().items() if v.dtype.is_floating_point})
        save_np(sd, str(dst))
        dst.with_suffix(".names.yaml").write_text(yaml.safe_dump({int(k): str(v) for k, v in yolo.names.items()}))
        print(f"wrote {dst} ({len(sd)} tensors, both head pairs) and {dst.with_suffix('.names.yaml')}")
        return
    net = yolo.model.float().fuse().eval()
    sd = {k: v.detach().float().contiguous() for k, v in net.state_dict().items()
          if v.dtype.is_floating_point and "dfl" not in k and "num_batches_tracked" not in k}
    dec = net.model[-1]
    if type(dec).__name__ == "RTDETRDecoder":
        import torch

        layer = dec.decoder.layers[0]
        aifi = next((m for m in net.model if type(m).__name__ == "AIFI"), None)
        sd["rtdetr.meta"] = torch.tensor([float(layer.cross_attn.n_heads), float(layer.cross_attn.n_points), float(dec.num_queries),
                                          float(aifi.ma.num_heads if aifi is not None else 8)])
    if type(dec).__name__ == "Classify":              # a ReID network (`with_reid: true, model: <file>`): its input size, default 224
        import torch

        sd["cls.meta"] = torch.tensor([float(yolo.model.args.get("imgsz", 224) if isinstance(getattr(yolo.model, "args", None), dict) else 224)])
    save_file(sd, str(dst))
    dst.with_suffix(".names.yaml").write_text(yaml.safe_dump({int(k): str(v) for k, v in yolo.names.items()}))
    print(f"wrote {dst} ({len(sd)} tensors) and {dst.with_suffix('.names.yaml')}")


if __name__ == "__main__":
    main()
