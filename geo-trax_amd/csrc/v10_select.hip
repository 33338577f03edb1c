// The YOLOv10 pass tail (v10Detect's one-to-one head, no NMS). gfx950.
//
// ultralytics' v10Detect.postprocess keeps Detect.max_det = 300 (kV10Keep) rows per image in two stages: the 300 anchors with the
// largest row-maximum class score, then the 300 largest of their 300 x nc scores; the predictor then gates score > conf, keeps
// `classes`, cuts to `max_det` and scales the boxes to the frame. Gating at conf first changes nothing (what the cut keeps of the
// gated entries is what the gate keeps of the cut), so the tail here is
//   head_candidates_kernel (every class kept)   anchors whose best score clears conf -> the candidate arrays, at most one per anchor
//   v10_select_kernel                          stage 1 over the candidates, the nc scores of the anchors kept (the gate's own
//                                              cls_scores4, head_device.hpp), stage 2 over them; the rows sorted by score
//   head_sparse_box_kernel / head_boxes_kernel the one-to-one box branch at the at most 300 entries kept
//   v10_rows_kernel                            `classes`, the max_det cut, scale_boxes + clip, the result rows
// in place of head_candidates -> head_sparse_box -> nms_small. Without ties the two stages equal one global top-300 over all
// anchors x nc scores (an entry inside the global top-k has fewer than k rows with a larger maximum; tests/test_yolov10.py shows it
// on seeded tensors). Tie rule, both stages: the lower index first -- the anchor index in stage 1, the flat index anchor * nc +
// class in stage 2 (torch.topk leaves ties unspecified). A candidate buffer holds every anchor, so nothing can overflow, and the
// box branch never sees more than 300 anchors: the dense box layers run for the debug read-backs only.
#include <hip/hip_runtime.h>
#include <hip/hip_fp16.h>

#include "det_kernels.hpp"
#include "head_device.hpp"

namespace gtx {

namespace {

__device__ __forceinline__ unsigned long long entry_key(float score, unsigned index) {   // larger score first, then the lower index
  return ((unsigned long long)__float_as_uint(score) << 32) | (unsigned long long)(0xFFFFFFFFu - index);   // scores are positive: their bits are monotone
}

// The want-th largest of the keys key(0 .. m - 1) (distinct, or 0 = no entry), by an 8-bit MSB-first radix select of the whole
// workgroup: the entries to keep are those with key >= the returned value and key != 0 (fewer than `want` exist: 0 comes back).
template <class KeyFn>
__device__ unsigned long long select_threshold(int m, int want, KeyFn key, unsigned* hist, unsigned long long* s_prefix, unsigned* s_need) {
  const int tid = threadIdx.x;
  if (tid == 0) { *s_prefix = 0ull; *s_need = (unsigned)want; }
  __syncthreads();
  unsigned long long mask = 0ull;
  for (int shift = 56; shift >= 0; shift -= 8) {
    if (tid < 256) hist[tid] = 0;
    __syncthreads();
    const unsigned long long prefix = *s_prefix;
    unsigned cur = 0xFFFFFFFFu, cnt = 0;               // a thread's consecutive keys mostly share the bin: one LDS atomic per run
    for (int i = tid; i < m; i += blockDim.x) {
      const unsigned long long k = key(i);
      if ((k & mask) != prefix) continue;
      const unsigned bin = (unsigned)(k >> shift) & 255u;
      if (bin == cur) { ++cnt; continue; }
      if (cnt) atomicAdd(&hist[cur], cnt);
      cur = bin;
      cnt = 1;
    }
    if (cnt) atomicAdd(&hist[cur], cnt);
    __syncthreads();
    if (tid == 0) {
      unsigned need = *s_need, b = 255;
      for (;; --b) {
        if (hist[b] >= need || b == 0) break;
        need -= hist[b];
      }
      *s_need = need;
      *s_prefix = prefix | ((unsigned long long)b << shift);
    }
    mask |= 255ull << shift;
    __syncthreads();
  }
  return *s_prefix;
}

constexpr int kSelThreads = 1024;
constexpr int kSortCap = 512;        // >= kV10Keep, a power of two

template <typename T>
__global__ __launch_bounds__(kSelThreads) void v10_select_kernel(const HeadParams hp, const NmsBuffers cand, const NmsBuffers sel, float* __restrict__ scores_all,
                                                                    int* __restrict__ kept_anchor) {
  __shared__ unsigned hist[256];
  __shared__ unsigned long long s_prefix;
  __shared__ unsigned s_need, s_n;
  __shared__ int s_anchor[kSortCap];
  __shared__ unsigned long long s_key[kSortCap];
  const int n = blockIdx.x, tid = threadIdx.x;
  const int nc = hp.nc;
  const int cnt = min(cand.count[n], cand.cap);
  const size_t base = (size_t)n * cand.cap;
  if (tid == 0) s_n = 0;
  if (tid < kMaxLevels && sel.lvl_count) sel.lvl_count[n * kMaxLevels + tid] = 0;
  __syncthreads();

  // ---- stage 1: the kV10Keep candidates (anchors) with the largest best-class score
  auto key1 = [&](int i) { return entry_key(cand.cand_score[base + i], (unsigned)cand.cand_anchor[base + i]); };
  unsigned long long thr = 0ull;
  if (cnt > kV10Keep) thr = select_threshold(cnt, kV10Keep, key1, hist, &s_prefix, &s_need);   // cnt is the same for every thread
  for (int i = tid; i < cnt; i += kSelThreads) {
    if (key1(i) >= thr) {
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)kV10Keep) s_anchor[slot] = cand.cand_anchor[base + i];
    }
  }
  __syncthreads();
  const int K = min((int)s_n, kV10Keep);
  if (K == 0) {
    if (tid == 0) sel.count[n] = 0;
    return;
  }
  if (kept_anchor && tid < K) kept_anchor[(size_t)n * kV10Keep + tid] = s_anchor[tid];   // which anchor each row of `scores` belongs to (operator tests)

  // ---- every class score of the anchors kept: 16 lanes per anchor, 64 anchors per round (whole waves: the shuffles need all lanes)
  float* scores = scores_all + (size_t)n * kV10Keep * nc;
  {
    const int sub = tid & 15, grp = tid >> 4;
    for (int k0 = 0; k0 < K; k0 += kSelThreads / 16) {
      const int k = k0 + grp;
      const int a = s_anchor[min(k, K - 1)];
      const HeadLevel& L = hp.lv[find_level(hp, a)];
      const T* fc = static_cast<const T*>(L.feat) + ((size_t)n * L.h * L.w + (a - L.anchor_begin)) * L.cstride + L.cb;
      for (int c0 = 0; c0 < nc; c0 += 4) {
        float sc[4];
        cls_scores4<T>(L, fc, sub, c0, nc, sc);
        if (sub == 0 && k < K) {
#pragma unroll
          for (int j = 0; j < 4; ++j)
            if (c0 + j < nc) scores[(size_t)k * nc + c0 + j] = sc[j];
        }
      }
    }
  }
  __syncthreads();                                    // the scores above are read by other threads of this workgroup below

  // ---- stage 2: the kV10Keep largest of the K x nc scores that clear conf
  const int M = K * nc;
  auto key2 = [&](int i) {
    const float sc = scores[i];
    const int k = i / nc;
    return sc > hp.conf ? entry_key(sc, (unsigned)s_anchor[k] * (unsigned)nc + (unsigned)(i - k * nc)) : 0ull;
  };
  thr = 0ull;
  if (M > kV10Keep) thr = select_threshold(M, kV10Keep, key2, hist, &s_prefix, &s_need);
  if (tid == 0) s_n = 0;
  if (tid < kSortCap) s_key[tid] = 0ull;
  __syncthreads();
  for (int i = tid; i < M; i += kSelThreads) {
    const unsigned long long k = key2(i);
    if (k != 0ull && k >= thr) {
      const unsigned slot = atomicAdd(&s_n, 1u);
      if (slot < (unsigned)kV10Keep) s_key[slot] = k;
    }
  }
  __syncthreads();
  const int kept = min((int)s_n, kV10Keep);
  for (int k = 2; k <= kSortCap; k <<= 1)             // bitonic, descending; the zero keys sink to the end
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (tid < kSortCap / 2) {
        const int lo = ((tid / j) * 2 * j) + (tid % j), hi = lo + j;
        const bool desc = ((lo & k) == 0);
        const unsigned long long a = s_key[lo], b = s_key[hi];
        if ((a < b) == desc) { s_key[lo] = b; s_key[hi] = a; }
      }
      __syncthreads();
    }
  if (tid < kept) {
    const unsigned long long k = s_key[tid];
    const unsigned flat = 0xFFFFFFFFu - (unsigned)(k & 0xFFFFFFFFull);
    const int a = (int)(flat / (unsigned)nc), c = (int)(flat - (unsigned)a * (unsigned)nc);
    const size_t o = (size_t)n * sel.cap + tid;
    sel.cand_score[o] = __uint_as_float((unsigned)(k >> 32));
    sel.cand_anchor[o] = a;
    sel.cand_cls[o] = c;
    if (sel.lvl_count) {                              // filed under its level for the sparse box branch (kept <= kV10Keep <= lvl_cap)
      const int l = find_level(hp, a);
      const int q = atomicAdd(&sel.lvl_count[n * kMaxLevels + l], 1);
      sel.lvl_list[((size_t)n * kMaxLevels + l) * sel.lvl_cap + q] = tid;
    }
  }
  if (tid == 0) sel.count[n] = kept;
}

// The rows of image n in score order: `classes`, the max_det cut, ultralytics' scale_boxes + clip_boxes (undo_letterbox)
__global__ __launch_bounds__(kSortCap) void v10_rows_kernel(const NmsBuffers sel, unsigned long long mask0, unsigned long long mask1, float gain, float padx,
                                                            float pady, float fw, float fh) {
  __shared__ int wave_cnt[kSortCap / 64];
  const int n = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cnt = min(sel.count[n], sel.cap);
  const size_t o = (size_t)n * sel.cap + tid;
  int c = 0;
  bool keep = false;
  if (tid < cnt) {
    c = sel.cand_cls[o];
    keep = c < 128 && (((c < 64 ? mask0 : mask1) >> (c & 63)) & 1ull);
  }
  const unsigned long long bal = __ballot(keep);
  if (lane == 0) wave_cnt[wave] = __popcll(bal);
  __syncthreads();
  int slot = __popcll(bal & ((1ull << lane) - 1ull)), total = 0;
  for (int w = 0; w < kSortCap / 64; ++w) {
    if (w < wave) slot += wave_cnt[w];
    total += wave_cnt[w];
  }
  if (keep && slot < sel.max_det) {
    float4 b = reinterpret_cast<const float4*>(sel.cand_box)[o];
    undo_letterbox(b, gain, padx, pady, fw, fh);
    float* r = sel.out_rows + ((size_t)n * sel.max_det + slot) * 6;
    r[0] = b.x; r[1] = b.y; r[2] = b.z; r[3] = b.w;
    r[4] = sel.cand_score[o];
    r[5] = (float)c;
    if (sel.out_anchor) sel.out_anchor[(size_t)n * sel.max_det + slot] = sel.cand_anchor[o];
  }
  if (tid == 0) sel.out_n[n] = min(total, sel.max_det);
}

}  // namespace

void launch_v10_select(int dtype, const HeadParams& hp, int n, const NmsBuffers& cand, const NmsBuffers& sel, float* scores, hipStream_t s, int* kept_anchor) {
  GTX_CHECK(sel.cap >= kV10Keep && sel.cap <= kSortCap && (!sel.lvl_count || sel.lvl_cap >= kV10Keep), "v10_select: the selection buffers hold %d entries", sel.cap);
  GTX_CHECK((long long)hp.n_anchors * hp.nc < (1ll << 32), "v10_select: %d anchors x %d classes do not fit a 32-bit flat index", hp.n_anchors, hp.nc);
  if (dtype == DT_F16) hipLaunchKernelGGL(v10_select_kernel<_Float16>, dim3(n), dim3(kSelThreads), 0, s, hp, cand, sel, scores, kept_anchor);
  else hipLaunchKernelGGL(v10_select_kernel<float>, dim3(n), dim3(kSelThreads), 0, s, hp, cand, sel, scores, kept_anchor);
  GTX_HIP(hipGetLastError());
}

void launch_v10_rows(const NmsBuffers& sel, const unsigned long long class_mask[2], int n, const Letterbox& lb, hipStream_t s) {
  const LetterboxUndo lu = letterbox_undo(lb);
  hipLaunchKernelGGL(v10_rows_kernel, dim3(n), dim3(kSortCap), 0, s, sel, class_mask[0], class_mask[1], lu.gain, lu.padx, lu.pady, lu.fw, lu.fh);
  GTX_HIP(hipGetLastError());
}

}  // namespace gtx
