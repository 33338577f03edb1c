// The YOLO detector's runtime around its graph (YOLOv8 / P2, YOLOv9, YOLOv10, YOLO11, YOLO26 `detect` checkpoints): the plan that
// computes the letterbox's padding rows once, finalize() with the post-pass workspaces, the post-pass itself (score gate, box
// branch, NMS or the one-to-one head's top-300 cut, result copies), what collect() finishes for a batch the pass left short, and
// the debug read-backs. The graph is built in detect_head.cpp: the trunk through yolo_trunk.cpp, then the Detect head.
#include "detector.hpp"

#include <algorithm>

namespace gtx {

Detector::Detector(gtx_ctx* ctx, const gtx_det_config& cfg)
    : DetectorBase(ctx, cfg, cfg.half ? DT_F16 : (cfg.fp32_split ? DT_F32S : DT_F32), dtype_size(cfg.half ? DT_F16 : DT_F32),
                   cfg.half ? DT_F16 : DT_F32),
      trunk_(*this, ops_, cfg.half ? DT_F16 : DT_F32) {
  dtype_ = cfg.half ? DT_F16 : DT_F32;
  es_ = dtype_size(dtype_);
  lb_ = letterbox_geometry(cfg.frame_h, cfg.frame_w, cfg.imgsz, cfg.rect != 0, 32);
  GTX_CHECK(lb_.net_h % 32 == 0 && lb_.net_w % 32 == 0, "network input %dx%d is not stride aligned", lb_.net_h, lb_.net_w);
}

Detector::~Detector() {
  if (h_feats_) (void)hipHostFree(h_feats_);
  if (h_count_) (void)hipHostFree(h_count_);
}

std::unique_ptr<NetRuntime> Detector::make_exact() const {
  gtx_det_config c = cfg_;
  c.fp32_split = 0;
  return std::unique_ptr<NetRuntime>(new Detector(ctx_, c));
}

void Detector::set_batch(int nb) {
  if (nb == cur_nb_) return;
  set_batch_ops(ops_, nb, es_, pad_skip_on_);
  cur_nb_ = nb;
}

// Rows of every activation tensor that can depend on the frame. The letterbox puts the resized frame in rows [top, top + new_h)
// of the network input and a constant colour everywhere else (ultralytics LetterBox, default.yaml `rect: false`: 420 + 420 of
// 1920 rows for a 16:9 frame); a convolution's output row outside the reach of those rows sees the same inputs for every
// frame, so its value is a constant of the checkpoint. Those rows are computed once (prime_pad_skip, at finalize) and the
// launches of every later pass cover the other tile rows only -- the buffers keep the constants, the results are the full
// launches' bit for bit. The interval grows with every 3x3 layer and covers the whole map from the SPPF on; the gain is in the
// backbone's large maps. GTX_PAD_SKIP=0: off.
void Detector::plan_pad_skip() {
  pad_skip_rows_ = pad_skip_total_ = 0;
  struct Rows { int lo, hi; };
  std::map<const void*, Rows> dep;                   // buffer -> frame-dependent rows; a buffer that is not here depends on the frame everywhere
  std::set<const void*> full;                        // ... and these stay that way whatever is written to them later
  // A region two different launches write (a scratch buffer reused by two layers) cannot keep either's constants: whoever
  // writes it computes every row. Writers per buffer as channel ranges.
  struct Writer { int c0, c1; Op* op; int member; };
  std::map<const void*, std::vector<Writer>> writers;
  auto second_writer = [&](const void* p, int c0, int c1, Op* op, int member) {
    bool hit = false;
    for (Writer& w : writers[p])
      if (c0 < w.c1 && w.c0 < c1) {
        hit = true;
        if (w.op->ty_count[w.member] > 0) {            // the earlier writer had been given a row range: take it back
          const ConvProblem& q = w.op->grp.p[w.member];
          pad_skip_rows_ -= (q.Ho + w.op->cfg.th - 1) / w.op->cfg.th - w.op->ty_count[w.member];
          w.op->ty_first[w.member] = w.op->ty_count[w.member] = 0;
        }
      }
    writers[p].push_back(Writer{c0, c1, op, member});
    return hit;
  };
  dep[img_.ptr] = Rows{lb_.top, lb_.top + lb_.new_h};
  auto through = [](Rows r, int k, int s, int h_out, int pad = -1) {   // rows of a k x k / stride s / pad k/2 (or `pad`) layer's output that see input rows [lo, hi)
    const int p = pad < 0 ? k / 2 : pad;
    const int num = r.lo + p - k + 1;                      // y >= num / s
    const int lo = num <= 0 ? 0 : (num + s - 1) / s;
    const int hi = (r.hi - 1 + p) / s + 1;
    return Rows{lo, std::min(h_out, hi)};
  };
  auto unite = [](Rows a, Rows b) { return Rows{std::min(a.lo, b.lo), std::max(a.hi, b.hi)}; };
  auto get = [&](const void* p, Rows& r) {
    auto it = dep.find(p);
    if (it == dep.end()) return false;
    r = it->second;
    return true;
  };
  auto put = [&](const void* p, bool known, Rows r) {
    if (!known) { dep.erase(p); full.insert(p); return; }
    if (full.count(p)) return;
    auto it = dep.find(p);
    if (it == dep.end()) dep[p] = r; else it->second = unite(it->second, r);   // another slice of a concat buffer may reach further
  };
  for (Op& op : ops_) {
    if (op.kind == Op::STEM) {
      Rows in{0, 0};
      const bool known = get(op.in.ptr, in);
      // yolov5.yaml's 6x6 / 2 / pad 2 stem: output row y reads image rows 2 y - 2 .. 2 y + 3
      put(op.out.ptr, known, op.stem_k == 6 ? through(in, 6, 2, op.out.h, 2) : through(in, 3, 2, op.out.h));
      continue;
    }
    if (op.kind != Op::CONV) { put(op.out.ptr, false, Rows{0, 0}); continue; }   // pools / upsampling: deep in the network
    for (int i = 0; i < op.grp.count; ++i) {
      const ConvProblem& p = op.grp.p[i];
      op.ty_first[i] = op.ty_count[i] = 0;
      Rows in{0, p.H};
      bool known;
      if (p.front_img) {
        Rows img{0, 0};
        known = get(p.front_img, img);
        if (known) in = through(img, 3, 2, p.H);
      } else {
        known = get(p.in, in) && p.c_split == 0;       // a second, upsampled source: neck layers, all rows
      }
      Rows out = through(in, op.cfg.ks, op.cfg.stride, p.Ho);
      if (known && p.res) {
        Rows r{0, 0};
        known = get(p.res, r);
        if (known) out = unite(out, r);
      }
      const int tiles = (p.Ho + op.cfg.th - 1) / op.cfg.th;
      pad_skip_total_ += tiles;
      if (second_writer(p.out, p.out_coff, p.out_coff + p.Cout, &op, i)) known = false;
      put(p.out, known, out);
      if (!known) continue;
      const int t0 = out.lo / op.cfg.th, t1 = std::min(tiles, (out.hi + op.cfg.th - 1) / op.cfg.th);
      if (t1 - t0 < tiles && t1 > t0) {
        op.ty_first[i] = t0;
        op.ty_count[i] = t1 - t0;
        pad_skip_rows_ += tiles - (t1 - t0);
      }
    }
  }
}

// One full pass over every batch slot on a blank frame: the rows the later launches skip now hold their constants.
void Detector::prime_pad_skip() {
  if (pad_skip_rows_ == 0) return;
  const int N = cfg_.max_batch;
  hipStream_t s = ctx_->stream;
  DevBuf blank;
  blank.alloc((size_t)N * cfg_.frame_h * cfg_.frame_w * 3);
  GTX_HIP(hipMemsetAsync(blank.p, 0, blank.bytes, s));
  pad_skip_on_ = false;
  cur_nb_ = 0;
  set_batch(N);
  launch_preprocess(dtype_, (const uint8_t*)blank.p, N, lb_, img_.ptr, nullptr, cfg_.frame_h / 2, cfg_.frame_w / 2, s);
  for (const Op& op : ops_) run_op(op, N, s);
  int sat = 0;
  if (sat_dev_) GTX_HIP(hipMemcpyAsync(&sat, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
  GTX_HIP(hipStreamSynchronize(s));
  cur_nb_ = 0;
  if (sat_dev_) GTX_HIP(hipMemsetAsync(sat_dev_, 0, sizeof(int), s));
  if (sat) {
    // A constant of the padding rows lies beyond fp16's range: it was clamped on its way into the pair format. With the rows
    // left out of the later launches no pass would raise the flag for them again, so the skipping stays off for this detector:
    // every pass computes (and checks) every row, and the first one falls back to the exact-fp32 kernels (collect()).
    pad_skip_on_ = false;
    pad_skip_rows_ = 0;
    for (Op& op : ops_)
      for (int i = 0; i < kMaxGroup; ++i) op.ty_first[i] = op.ty_count[i] = 0;
    return;
  }
  pad_skip_on_ = true;
}

// The sparse box branch files its candidates by level: the lists in b, `cap` entries per level and image
void Detector::alloc_level_lists(NmsBuffers& b, int cap) {
  sparse_.cap = cap;
  sparse_.sat_flag = sat_dev_;
  b.lvl_cap = cap;
  b.lvl_count = (int*)alloc(sizeof(int) * cfg_.max_batch * kMaxLevels);
  b.lvl_list = (int*)alloc(sizeof(int) * cfg_.max_batch * kMaxLevels * cap);
}

void Detector::finalize() {
  GTX_CHECK(!finalized_, "finalize called twice");
  GTX_HIP(hipSetDevice(ctx_->device));
  build_graph();
  trunk_.fuse();
  const int N = cfg_.max_batch;
  alloc_outputs();
  // NMS workspace. Candidate capacity = every anchor; sort/NMS capacity = ultralytics max_nms.
  nms_ = NmsBuffers{};
  nms_.cap = head_.n_anchors;
  nms_.nms_cap = 30016;  // >= max_nms (30000), multiple of 64
  nms_.max_det = cfg_.max_det;
  nms_.count = (int*)alloc(sizeof(int) * N);
  nms_.cand_score = (float*)alloc(sizeof(float) * N * nms_.cap);
  nms_.cand_anchor = (int*)alloc(sizeof(int) * N * nms_.cap);
  nms_.cand_cls = (int*)alloc(sizeof(int) * N * nms_.cap);
  nms_.cand_box = (float*)alloc(sizeof(float) * 4 * N * nms_.cap);
  if (!end2end_) {                                   // the sort / mask workspace of the NMS kernels (113 MB per batch slot): the one-to-one head runs none of them
    nms_.sorted_n = (int*)alloc(sizeof(int) * N);
    nms_.s_box = (float*)alloc(sizeof(float) * 4 * N * nms_.nms_cap);
    nms_.s_score = (float*)alloc(sizeof(float) * N * nms_.nms_cap);
    nms_.s_cls = (int*)alloc(sizeof(int) * N * nms_.nms_cap);
    nms_.mask = (unsigned long long*)alloc(sizeof(unsigned long long) * N * (size_t)nms_.nms_cap * (nms_.nms_cap / 64));
  }
  nms_.out_n = (int*)alloc(sizeof(int) * N);
  nms_.out_rows = (float*)alloc(sizeof(float) * 6 * N * cfg_.max_det);
  nms_.s_anchor = nms_.out_anchor = nullptr;
  if (cfg_.obj_feats) {
    nms_.s_anchor = (int*)alloc(sizeof(int) * N * nms_.nms_cap);
    nms_.out_anchor = (int*)alloc(sizeof(int) * N * cfg_.max_det);
    d_feats_ = (float*)alloc(sizeof(float) * N * cfg_.max_det * feat_levels_.dim);
    GTX_HIP(hipHostMalloc((void**)&h_feats_, sizeof(float) * N * cfg_.max_det * feat_levels_.dim));
  }
  if (sparse_on_ && !end2end_) alloc_level_lists(nms_, kSparseCap);
  if (end2end_) {
    // the one-to-one head: nms_ holds the gate's candidates (one per anchor at most); sel_ the entries v10_select keeps, with the
    // result buffers; the box branch runs on sel_'s entries only
    sel_ = nms_;
    sel_.cap = kSelCap;
    sel_.count = (int*)alloc(sizeof(int) * N);
    sel_.cand_score = (float*)alloc(sizeof(float) * N * kSelCap);
    sel_.cand_anchor = (int*)alloc(sizeof(int) * N * kSelCap);
    sel_.cand_cls = (int*)alloc(sizeof(int) * N * kSelCap);
    sel_.cand_box = (float*)alloc(sizeof(float) * 4 * N * kSelCap);
    if (sparse_on_) alloc_level_lists(sel_, kSelCap);   // nms_, the gate's buffer, keeps none
    v10_scores_ = (float*)alloc(sizeof(float) * N * kV10Keep * cfg_.nc);
  }
  GTX_HIP(hipHostMalloc((void**)&h_count_, sizeof(int) * N));
  drop_tensors_unless_fallback();
  if (env_flag("GTX_PAD_SKIP", true)) {
    plan_pad_skip();
    prime_pad_skip();
  }
  set_batch(1);
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  finalized_ = true;
}

void Detector::run_op(const Op& op, int nb, hipStream_t s) { trunk_.run_op(op, nb, s); }

void Detector::run_post(int nb, hipStream_t s) {
  if (end2end_) {                                  // no NMS: gate -> the two-stage top-300 cut -> the box branch at the entries kept -> rows
    HeadParams gate = head_;
    gate.class_mask[0] = gate.class_mask[1] = ~0ull;   // `classes` is applied to the rows the cut keeps, not in front of it
    launch_head_gate(dtype_, gate, nb, nms_, s);
    launch_v10_select(dtype_, head_, nb, nms_, sel_, v10_scores_, s);
    if (sparse_on_) {
      launch_head_sparse_box(sparse_, nb, sel_, s);
      dense_head_valid_ = false;
    } else {
      launch_head_boxes(dtype_, head_, nb, sel_, s);
    }
    launch_v10_rows(sel_, head_.class_mask, nb, lb_, s);
  } else if (sparse_on_) {                         // score gate -> the box branch at the candidates -> their boxes
    launch_head_gate(dtype_, head_, nb, nms_, s);
    launch_head_sparse_box(sparse_, nb, nms_, s);
    dense_head_valid_ = false;
  } else {
    launch_head_candidates(dtype_, head_, nb, nms_, s);
  }
  // the candidate counts come back with the results: collect() runs what this pass leaves out for a batch that needs it (the
  // general NMS kernels for > 4096 candidates in an image, the dense box layers for > kSparseCap)
  GTX_HIP(hipMemcpyAsync(h_count_, nms_.count, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
  if (!end2end_) launch_nms(nms_, nb, cfg_.iou, cfg_.agnostic_nms != 0, 30000, lb_, s, 1);
  read_back(end2end_ ? sel_ : nms_, nb, true, s);
}

void Detector::read_back(const NmsBuffers& r, int nb, bool sat, hipStream_t s) {
  GTX_HIP(hipMemcpyAsync(h_out_n_, r.out_n, sizeof(int) * nb, hipMemcpyDeviceToHost, s));
  GTX_HIP(hipMemcpyAsync(h_out_rows_, r.out_rows, sizeof(float) * 6 * nb * cfg_.max_det, hipMemcpyDeviceToHost, s));
  if (sat && sat_dev_) GTX_HIP(hipMemcpyAsync(h_sat_, sat_dev_, sizeof(int), hipMemcpyDeviceToHost, s));
  if (!cfg_.obj_feats) return;                     // never with the one-to-one head (choose_head_pair)
  launch_obj_feats(fmt_, feat_levels_, nb, r, d_feats_, s);
  GTX_HIP(hipMemcpyAsync(h_feats_, d_feats_, sizeof(float) * nb * cfg_.max_det * feat_levels_.dim, hipMemcpyDeviceToHost, s));
}

// The dense box layers of the Detect head on the activations of the pass that ran last (sparse mode leaves them out of the
// forward): for the debug read-backs and for a batch with more candidates than the sparse buffer holds.
void Detector::run_dense_box(hipStream_t s) {
  if (!sparse_on_ || dense_head_valid_) return;
  GTX_CHECK(cur_nb_ > 0, "no forward pass has run yet");
  for (Op o : dense_box_ops_) {
    for (int i = 0; i < o.grp.count; ++i) o.grp.p[i].N = cur_nb_;
    conv_group_finalize(o.grp, o.cfg);
    run_op(o, cur_nb_, s);
  }
  dense_head_valid_ = true;
}

// What the pass left out for the common case: the general NMS kernels for > 4096 candidates in an image, the dense box layers and
// every candidate's box for > kSparseCap; then the appearance vectors out of the pinned buffer before the next pass lands in it.
void Detector::after_pass(int nb) {
  // The one-to-one head leaves nothing out of its pass, so there is no overflow case to finish here: the gate's buffer (nms_.cap =
  // n_anchors) takes one candidate per anchor at most, head_candidates_kernel writes no more, and v10_select hands the box branch at
  // most kV10Keep = 300 entries of sel_'s 304 (cap and lvl_cap) -- the sparse buffer cannot fill, whatever conf is
  // (tests/test_yolov10_gpu.py::test_every_anchor_a_candidate). No NMS runs either, so there is no large-NMS re-run.
  if (end2end_) return;
  bool over = false, big = false;
  for (int b = 0; b < nb; ++b) {
    over = over || (sparse_on_ && h_count_[b] > kSparseCap);                 // more candidates than the sparse buffer holds
    big = big || !nms_small_covers(std::min(h_count_[b], nms_.cap), nms_.max_det);   // ... than the single-workgroup NMS takes
  }
  if (over || big) {
    hipStream_t s = ctx_->stream;
    if (over) {                                      // the dense box layers, then every candidate's box again
      run_dense_box(s);
      launch_head_boxes(dtype_, head_, nb, nms_, s);
      ++sparse_overflows_;
    }
    launch_nms(nms_, nb, cfg_.iou, cfg_.agnostic_nms != 0, 30000, lb_, s, over ? 0 : 2);
    read_back(nms_, nb, false, s);                   // the flag has come back with the pass
    record_post_end(s);                              // the postprocess figure now includes the re-run
    GTX_HIP(hipStreamSynchronize(s));
  }
  if (cfg_.obj_feats) {
    c_feat_n_.assign(cfg_.max_batch, 0);
    c_feats_.resize((size_t)cfg_.max_batch * cfg_.max_det * feat_levels_.dim);
    for (int b = 0; b < nb; ++b) {
      c_feat_n_[b] = h_out_n_[b];
      const size_t o = (size_t)b * cfg_.max_det * feat_levels_.dim;
      memcpy(c_feats_.data() + o, h_feats_ + o, sizeof(float) * h_out_n_[b] * feat_levels_.dim);
    }
  }
}

void Detector::features(int b, float* out, int cap, int* n, int* dim) const {
  GTX_CHECK(cfg_.obj_feats && h_feats_, "features: the detector was created without gtx_det_config.obj_feats");
  GTX_CHECK(b >= 0 && b < cfg_.max_batch, "features: image %d of %d", b, cfg_.max_batch);
  const int cnt = std::min(b < (int)c_feat_n_.size() ? c_feat_n_[b] : 0, cap);
  if (n) *n = cnt;
  if (dim) *dim = feat_levels_.dim;
  if (out && cnt > 0) memcpy(out, c_feats_.data() + (size_t)b * cfg_.max_det * feat_levels_.dim, sizeof(float) * cnt * feat_levels_.dim);
}

void Detector::raw_output(int b, float* out, int* n_anchors, bool logits) {
  GTX_CHECK(finalized_ && cur_nb_ > 0 && b >= 0 && b < cur_nb_, "raw_output: no forward pass for slot %d", b);
  const size_t per = (size_t)head_.n_anchors * (4 + head_.nc);
  if (raw_.bytes < per * cur_nb_ * sizeof(float)) raw_.alloc(per * cur_nb_ * sizeof(float));
  GTX_CHECK(!in_flight_, "raw_output while a batch is in flight: call collect first");
  run_dense_box(ctx_->stream);                     // the full decode reads every anchor's box features
  launch_head_raw(dtype_, head_, cur_nb_, raw_.as<float>(), logits, ctx_->stream);
  GTX_HIP(hipMemcpyAsync(out, raw_.as<float>() + per * b, per * sizeof(float), hipMemcpyDeviceToHost, ctx_->stream));
  GTX_HIP(hipStreamSynchronize(ctx_->stream));
  if (n_anchors) *n_anchors = head_.n_anchors;
}

void Detector::layer_output(int b, const std::string& layer, float* out, int* h, int* w, int* c) {
  // Not while a pass is in flight: the stand-alone launches of the hidden layers would queue behind it and overwrite the
  // buffers it shares with them.
  GTX_CHECK(!(out && in_flight_), "layer_output while a batch is in flight: call collect first");
  auto it = layer_views_.find(layer);
  if (it == layer_views_.end()) fail(-1, "unknown layer '%s'", layer.c_str());
  const View& v = it->second;
  if (out && sparse_on_ && cur_nb_ > 0 && (layer.rfind(det_pfx_ + ".", 0) == 0 || layer.rfind("__head", 0) == 0)) {
    GTX_HIP(hipSetDevice(ctx_->device));
    run_dense_box(ctx_->stream);                   // the head's box layers are not part of the forward in sparse mode
    GTX_HIP(hipStreamSynchronize(ctx_->stream));
  }
  if (out) trunk_.recompute_hidden(layer, cur_nb_, ctx_->stream);   // the stem's output, model.1's: not written by the fused front
  if (h) *h = v.h;
  if (w) *w = v.w;
  if (c) *c = v.c;
  if (!out) return;
  GTX_CHECK(b >= 0 && b < cfg_.max_batch, "bad batch slot");
  GTX_CHECK(!trunk_.hidden(v.ptr), "layer_output('%s'): the layer's buffer was not re-created", layer.c_str());
  read_view(v, b, out);
}

}  // namespace gtx
