// The YOLO trunks' layer tables and the pure host arithmetic around them: no HIP, no device memory, so that the host sanitizer
// builds (make asan tsan, csrc/hosttest/sanitize_host.cpp) cover them. yolo_trunk.cpp walks the tables.
#pragma once
#include <cstddef>
#include <vector>

namespace gtx {

// One row of a trunk's layer table: a layer of the model yaml, as the yaml writes it
struct TrunkRow {
  enum Module { CONV, BLOCK, SPPF, C2PSA, UPSAMPLE, CONCAT, DETECT, SCDOWN, PSA, ELAN, ADOWN, SPPELAN, A2C2F, C3 };
  int i;            // the layer index: its tensors are "model.<i>.*"
  Module mod;       // CONV: Conv 3x3 stride 2, or 1x1 stride 1 (yolov5.yaml's neck; the tensor tells), row 0: the stem (3x3, or yolov5.yaml's
                    // 6x6 / 2 / pad 2; the tensor tells); BLOCK: C2f / C3k2 / C2fCIB (which one, the tensors tell);
                    // SCDOWN: 1x1 Conv + depthwise 3x3 stride 2 without activation; PSA: C2PSA's one block directly under the layer (yolov10.yaml);
                    // ELAN: ELAN1 / RepNCSPELAN4, ADOWN: AConv / ADown (which one, the tensors tell), SPPELAN: SPPF's pools closed by cv5 (yolov9.yaml);
                    // A2C2F: yolo12.yaml's block, members of two ABlocks (area attention) or one C3k each (which, the tensors tell)
                    // C3: yolov5.yaml's block, cv3(cat(m(cv1 x), cv2 x)) with m = Bottlenecks (1x1, 3x3) of full hidden width
  int from[4];      // the yaml's `from`: -1 = the row above (row 0: the image), else a layer index; 0 ends the list
  bool shortcut;    // BLOCK / C3: the bottlenecks add their input; SPPF: yolo26.yaml's form (cv1 without activation, the input added to cv2's output)
  int area = 0;     // A2C2F with ABlocks: the yaml's `area` (bands the attention is cut into; 1 = the whole map). No tensor tells it.
};
struct TrunkGraph {
  const TrunkRow* rows;
  int n;
  bool dw_cls;      // yolo11.yaml's Detect: the class branch is DWConv + 1x1 Conv twice
};

// The first row of a table that build() cannot walk, -1 when there is none: row i is layer i, it reads at least one layer, only
// earlier ones (row 0: the image), a Concat's members feed one Concat only, an Upsample leads its Concat, the Detect row comes last.
inline int trunk_table_error(const TrunkRow* rows, int n) {
  std::vector<int> cat_of(n > 0 ? n : 0, -1);
  for (int i = 0; i < n; ++i) {
    const TrunkRow& r = rows[i];
    int nf = 0;
    while (nf < 4 && r.from[nf] != 0) ++nf;
    if (r.i != i || nf < 1) return i;
    for (int k = 0; k < nf; ++k) {
      const int f = r.from[k] < 0 ? i + r.from[k] : r.from[k];
      if (f >= i || (f < 0 && i != 0)) return i;
      if (r.mod == TrunkRow::CONCAT) {
        if (cat_of[f] >= 0 || (rows[f].mod == TrunkRow::UPSAMPLE && k != 0)) return i;
        cat_of[f] = i;
      }
    }
    if (r.mod == TrunkRow::DETECT && i != n - 1) return i;
    if (r.mod != TrunkRow::CONCAT && r.mod != TrunkRow::DETECT && nf != 1) return i;
  }
  return -1;
}

// Depthwise weights [C][1][k][k] (taps = k * k values per channel) -> tap-major [taps][C], what rt_dwconv_* read
inline std::vector<float> dw_tap_major(const float* w, int c, int taps) {
  std::vector<float> wt((size_t)taps * c);
  for (int ch = 0; ch < c; ++ch)
    for (int t = 0; t < taps; ++t) wt[(size_t)t * c + ch] = w[(size_t)ch * taps + t];
  return wt;
}

// Which kernel a launcher of rtdetr_kernels.hpp runs. The launcher dispatches on the predicate, the graph builders label their ops
// (OpInfo::family, what the profile tables are keyed by) with the name.
// launch_rt_dwconv: the LDS-tiled form at stride 1 on whole 32-channel groups (GTX_RT_DW_TILE=0, a debugging switch, aside)
inline bool rt_dwconv_tiled(int stride, int c) { return stride == 1 && c % 32 == 0; }
inline const char* rt_dwconv_kernel_name(int k, int stride, int c) {
  const bool t = rt_dwconv_tiled(stride, c);
  if (k == 3) return t ? "rt_dwconv_tile_kernel<3>" : "rt_dwconv_kernel<3>";
  if (k == 5) return t ? "rt_dwconv_tile_kernel<5>" : "rt_dwconv_kernel<5>";
  return t ? "rt_dwconv_tile_kernel<7>" : "rt_dwconv_kernel<7>";
}
// launch_psa_attention (form 0): maps of at most kPsaSmallT positions run the one-workgroup-per-(image, head) kernel
inline constexpr int kPsaSmallT = 64;
inline bool psa_attention_small(int h, int w) { return h * w <= kPsaSmallT; }
inline const char* psa_attention_kernel_name(int h, int w) { return psa_attention_small(h, w) ? "psa_attn_small_kernel" : "psa_attn_kernel"; }
// launch_area_attention (area_attn.hpp): keys per LDS stage of area_attn_kernel; a map runs when its positions cut into `area` equal runs
inline constexpr int kAreaAttnKeyTile = 64;
inline bool area_attention_fits(int h, int w, int area) { return area >= 1 && h >= 1 && w >= 1 && (h * w) % area == 0; }
// launch_stem6 (stem6.hpp): the output side of Conv(k = 6, s = 2, p = 2) on a side of `n` pixels (n >= 2), and the workgroup's tile of
// output pixels: rows x columns on the matrix-core kernels (one row per wave), rows x columns on the exact-fp32 kernel
inline int stem6_out(int n) { return (n - 2) / 2 + 1; }
inline constexpr int kStem6Cols = 32, kStem6Rows = 4, kStem6RowsF32 = 8;

namespace tables {
using R = TrunkRow;
inline constexpr R kYolov8[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::BLOCK, {-1}, true},       {7, R::CONV, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::SPPF, {-1}, false},        {10, R::UPSAMPLE, {-1}, false},  {11, R::CONCAT, {-1, 6}, false},
    {12, R::BLOCK, {-1}, false},    {13, R::UPSAMPLE, {-1}, false},   {14, R::CONCAT, {-1, 4}, false}, {15, R::BLOCK, {-1}, false},
    {16, R::CONV, {-1}, false},     {17, R::CONCAT, {-1, 12}, false}, {18, R::BLOCK, {-1}, false},     {19, R::CONV, {-1}, false},
    {20, R::CONCAT, {-1, 9}, false}, {21, R::BLOCK, {-1}, false},     {22, R::DETECT, {15, 18, 21}, false}};
inline constexpr int kClsBackboneRows = 9;   // yolov8-cls.yaml: model.0-8 are yolov8.yaml's
inline constexpr R kYolov8P2[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::BLOCK, {-1}, true},       {7, R::CONV, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::SPPF, {-1}, false},        {10, R::UPSAMPLE, {-1}, false},  {11, R::CONCAT, {-1, 6}, false},
    {12, R::BLOCK, {-1}, false},    {13, R::UPSAMPLE, {-1}, false},   {14, R::CONCAT, {-1, 4}, false}, {15, R::BLOCK, {-1}, false},
    {16, R::UPSAMPLE, {-1}, false}, {17, R::CONCAT, {-1, 2}, false},  {18, R::BLOCK, {-1}, false},     {19, R::CONV, {-1}, false},
    {20, R::CONCAT, {-1, 15}, false}, {21, R::BLOCK, {-1}, false},    {22, R::CONV, {-1}, false},      {23, R::CONCAT, {-1, 12}, false},
    {24, R::BLOCK, {-1}, false},    {25, R::CONV, {-1}, false},       {26, R::CONCAT, {-1, 9}, false}, {27, R::BLOCK, {-1}, false},
    {28, R::DETECT, {18, 21, 24, 27}, false}};
// YOLO11's shortcuts: on in the backbone; in the neck kNeckShortcut, which no tensor tells (taken as off, as in yolov8.yaml's neck;
// tests/yolo11_ref.py names the doubt).
inline constexpr bool kNeckShortcut = false;
inline constexpr R kYolo11[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::BLOCK, {-1}, true},       {7, R::CONV, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::SPPF, {-1}, false},        {10, R::C2PSA, {-1}, false},     {11, R::UPSAMPLE, {-1}, false},
    {12, R::CONCAT, {-1, 6}, false}, {13, R::BLOCK, {-1}, kNeckShortcut}, {14, R::UPSAMPLE, {-1}, false}, {15, R::CONCAT, {-1, 4}, false},
    {16, R::BLOCK, {-1}, kNeckShortcut}, {17, R::CONV, {-1}, false},  {18, R::CONCAT, {-1, 13}, false}, {19, R::BLOCK, {-1}, kNeckShortcut},
    {20, R::CONV, {-1}, false},     {21, R::CONCAT, {-1, 10}, false}, {22, R::BLOCK, {-1}, kNeckShortcut}, {23, R::DETECT, {16, 19, 22}, false}};
// v10/yolov10{n,s}.yaml: SCDown in place of the stride-2 Convs at 5 / 7 / 20, PSA = model.10, C2fCIB where the tensors say so (model.8
// of scale s, model.22), v10Detect = model.23: YOLO11's Detect layers twice (cv2 / cv3 and one2one_cv2 / one2one_cv3)
inline constexpr R kYolo10[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::SCDOWN, {-1}, false},      {6, R::BLOCK, {-1}, true},       {7, R::SCDOWN, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::SPPF, {-1}, false},        {10, R::PSA, {-1}, false},       {11, R::UPSAMPLE, {-1}, false},
    {12, R::CONCAT, {-1, 6}, false}, {13, R::BLOCK, {-1}, false},     {14, R::UPSAMPLE, {-1}, false},  {15, R::CONCAT, {-1, 4}, false},
    {16, R::BLOCK, {-1}, false},    {17, R::CONV, {-1}, false},       {18, R::CONCAT, {-1, 13}, false}, {19, R::BLOCK, {-1}, false},
    {20, R::SCDOWN, {-1}, false},   {21, R::CONCAT, {-1, 10}, false}, {22, R::BLOCK, {-1}, true},      {23, R::DETECT, {16, 19, 22}, false}};
// 26/yolo26.yaml: kYolo11's rows; SPPF(shortcut) = model.9 and, told by its tensors, the C3k2 with attention (m.{k} = Bottleneck + PSABlock)
// = model.22; Detect = model.23 with reg_max = 1 and a one-to-one pair (the 4-row last box convolution tells). What no tensor tells,
// tests/yolo26_ref.py lists as doubts: the neck's shortcuts (kNeckShortcut, as for YOLO11), model.22's Bottleneck shortcut (taken as on)
// and whether SPPF's residual follows cv2's activation (taken as so: the epilogue form proj / ffn.1 use; the other order is not built).
inline constexpr bool kAttnBlockShortcut = true;
inline constexpr bool kSppfResidualAfterAct = true;
static_assert(kSppfResidualAfterAct, "SPPF's residual in front of the activation is not built");
inline constexpr R kYolo26[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::BLOCK, {-1}, true},       {7, R::CONV, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::SPPF, {-1}, true},         {10, R::C2PSA, {-1}, false},     {11, R::UPSAMPLE, {-1}, false},
    {12, R::CONCAT, {-1, 6}, false}, {13, R::BLOCK, {-1}, kNeckShortcut}, {14, R::UPSAMPLE, {-1}, false}, {15, R::CONCAT, {-1, 4}, false},
    {16, R::BLOCK, {-1}, kNeckShortcut}, {17, R::CONV, {-1}, false},  {18, R::CONCAT, {-1, 13}, false}, {19, R::BLOCK, {-1}, kNeckShortcut},
    {20, R::CONV, {-1}, false},     {21, R::CONCAT, {-1, 10}, false}, {22, R::BLOCK, {-1}, kAttnBlockShortcut}, {23, R::DETECT, {16, 19, 22}, false}};
// v9/yolov9{t,s,m,c}.yaml: ELAN1 or RepNCSPELAN4 where the others have C2f, AConv (t / s / m) or ADown (c) where they have the
// stride-2 Convs, SPPELAN = model.9, YOLOv8's Detect = model.22
inline constexpr R kYolo9[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::ELAN, {-1}, true},        {3, R::ADOWN, {-1}, false},
    {4, R::ELAN, {-1}, true},       {5, R::ADOWN, {-1}, false},       {6, R::ELAN, {-1}, true},        {7, R::ADOWN, {-1}, false},
    {8, R::ELAN, {-1}, true},       {9, R::SPPELAN, {-1}, false},     {10, R::UPSAMPLE, {-1}, false},  {11, R::CONCAT, {-1, 6}, false},
    {12, R::ELAN, {-1}, true},      {13, R::UPSAMPLE, {-1}, false},   {14, R::CONCAT, {-1, 4}, false}, {15, R::ELAN, {-1}, true},
    {16, R::ADOWN, {-1}, false},    {17, R::CONCAT, {-1, 12}, false}, {18, R::ELAN, {-1}, true},       {19, R::ADOWN, {-1}, false},
    {20, R::CONCAT, {-1, 9}, false}, {21, R::ELAN, {-1}, true},       {22, R::DETECT, {15, 18, 21}, false}};
// 12/yolo12.yaml: 22 layers, no SPPF and no C2PSA; A2C2f with area attention at strides 16 (area 4) and 32 (area 1) of the backbone,
// A2C2f with C3k members in the neck, a C3k2 as the neck's last block, YOLO11's Detect = model.21. The C3k members of A2C2f take the
// module's default shortcut (on); tests/yolo12_ref.py lists the doubts.
inline constexpr bool kA2C2fC3kShortcut = true;
inline constexpr R kYolo12[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::A2C2F, {-1}, false, 4},   {7, R::CONV, {-1}, false},
    {8, R::A2C2F, {-1}, false, 1},  {9, R::UPSAMPLE, {-1}, false},    {10, R::CONCAT, {-1, 6}, false}, {11, R::A2C2F, {-1}, kA2C2fC3kShortcut},
    {12, R::UPSAMPLE, {-1}, false}, {13, R::CONCAT, {-1, 4}, false},  {14, R::A2C2F, {-1}, kA2C2fC3kShortcut}, {15, R::CONV, {-1}, false},
    {16, R::CONCAT, {-1, 11}, false}, {17, R::A2C2F, {-1}, kA2C2fC3kShortcut}, {18, R::CONV, {-1}, false}, {19, R::CONCAT, {-1, 8}, false},
    {20, R::BLOCK, {-1}, kNeckShortcut}, {21, R::DETECT, {14, 17, 20}, false}};
// v5/yolov5.yaml with the anchor-free Detect (the yolov5{n,s,m,l,x}u files): a 6x6 stem, C3 blocks (shortcut on in the backbone, off in the
// neck, as the yaml writes it), SPPF = model.9, 1x1 Convs at model.10 / 14 that feed both an Upsample and the Concats 22 / 19 of the way
// back down, YOLOv8's Detect = model.24. 25 layers. tests/yolov5u_ref.py lists the doubts.
inline constexpr R kYolov5u[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::C3, {-1}, true},          {3, R::CONV, {-1}, false},
    {4, R::C3, {-1}, true},         {5, R::CONV, {-1}, false},        {6, R::C3, {-1}, true},          {7, R::CONV, {-1}, false},
    {8, R::C3, {-1}, true},         {9, R::SPPF, {-1}, false},        {10, R::CONV, {-1}, false},      {11, R::UPSAMPLE, {-1}, false},
    {12, R::CONCAT, {-1, 6}, false}, {13, R::C3, {-1}, false},        {14, R::CONV, {-1}, false},      {15, R::UPSAMPLE, {-1}, false},
    {16, R::CONCAT, {-1, 4}, false}, {17, R::C3, {-1}, false},        {18, R::CONV, {-1}, false},      {19, R::CONCAT, {-1, 14}, false},
    {20, R::C3, {-1}, false},       {21, R::CONV, {-1}, false},       {22, R::CONCAT, {-1, 10}, false}, {23, R::C3, {-1}, false},
    {24, R::DETECT, {17, 20, 23}, false}};
// yolo11-cls.yaml: model.0-8 are yolo11.yaml's, C2PSA follows them directly (no SPPF) and is the embedded layer; Classify = model.10
inline constexpr R kYolo11Cls[] = {
    {0, R::CONV, {-1}, false},      {1, R::CONV, {-1}, false},        {2, R::BLOCK, {-1}, true},       {3, R::CONV, {-1}, false},
    {4, R::BLOCK, {-1}, true},      {5, R::CONV, {-1}, false},        {6, R::BLOCK, {-1}, true},       {7, R::CONV, {-1}, false},
    {8, R::BLOCK, {-1}, true},      {9, R::C2PSA, {-1}, false}};
template <int N> constexpr TrunkGraph graph_of(const R (&rows)[N], bool dw_cls) { return TrunkGraph{rows, N, dw_cls}; }
}  // namespace tables

}  // namespace gtx
