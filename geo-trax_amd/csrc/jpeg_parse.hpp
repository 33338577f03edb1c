// Host half of the JPEG frame source: marker walk and Huffman decode of one baseline JPEG (the compressed frame of a Motion-JPEG
// clip or of a folder of .jpg files) into a packed record of quantised coefficients. It replaces the entropy-decoding half of
// cv2.VideoCapture.read() (geotrax/extract.py:146); dequantisation, the inverse DCT, chroma upsampling and the colour conversion are
// csrc/jpeg.hip's. Plain C++, no HIP: it compiles alone (csrc/diag/jpeg_parse_check.cpp runs it under the sanitizers).
//
// Record (little endian, 4-byte aligned):
//   RecordHeader                       80 bytes
//   uint16 quant[3][64]                one table per component, natural (row-major) order
//   uint32 offset[n_blocks + 1]        offset[b] = index of block b's first coefficient in the stream, offset[n_blocks] = n_coef
//   int16  coef[n_coef]                per block: the quantised coefficients in zigzag order up to the last non-zero one, DC
//                                      prediction resolved; an all-zero block has length 0
// Blocks are numbered in scan order: MCU by MCU (raster over the MCU grid), inside an MCU the hs x vs luma blocks row by row, then
// Cb, then Cr. A one-component frame is a raster of single blocks over ceil(w/8) x ceil(h/8).
#pragma once
#include <cstddef>
#include <cstdint>

namespace gtx {
namespace jpeg {

constexpr uint32_t kMagic = 0x3152474au;      // "JGR1"
constexpr int kMaxDim = 16384;               // larger frames are refused (the record's 32-bit sizes)
constexpr int kOk = 0, kTooSmall = 1, kInvalid = -1, kUnsupported = -3;   // the negative ones are gtx_status values

struct RecordHeader {
  uint32_t magic, bytes;                     // bytes: the whole record
  uint32_t width, height, ncomp;             // ncomp 1 (grayscale) or 3 (YCbCr)
  uint32_t hs, vs;                           // luma sampling factors: 1x1, 2x1 or 2x2 (chroma is 1x1)
  uint32_t mcus_x, mcus_y;
  uint32_t n_blocks, n_coef;
  uint32_t bw[3], bh[3];                     // block grid of every component (MCU padding included)
  uint32_t reserved[3];
};
static_assert(sizeof(RecordHeader) == 80, "record header layout");
constexpr size_t kQuantOffset = sizeof(RecordHeader);
constexpr size_t kOffsetsOffset = kQuantOffset + 3 * 64 * sizeof(uint16_t);

inline size_t record_bytes(size_t n_blocks, size_t n_coef) { return kOffsetsOffset + 4 * (n_blocks + 1) + 2 * n_coef; }
// Most 8x8 blocks a frame of h x w can have, over the accepted samplings (MCU padding included).
size_t max_blocks(int h, int w);
// Largest record a frame of h x w can need, over the accepted samplings (every block 64 coefficients long).
size_t record_bound(int h, int w);
// Bytes of the u8 sample planes the first kernel writes for this record (Y, Cb, Cr at their padded block-grid sizes).
size_t planes_bytes(const RecordHeader& hd);

struct Info {
  int width = 0, height = 0, ncomp = 0, hs = 0, vs = 0;
};

// Decodes bytes[0, n) into `record` (capacity bytes, 4-byte aligned; may be NULL with capacity 0). *needed receives the record's
// size whenever the frame decodes. Returns kOk (record filled), kTooSmall (the frame decoded, the record was not written: call
// again with *needed bytes), kUnsupported (a variant outside the accepted set; msg names the marker) or kInvalid (damaged data).
// No byte outside bytes[0, n) is read and none outside record[0, capacity) written, whatever the data says. `frame` only
// numbers the frame in messages. *info is filled as soon as the frame header is read.
int parse(const uint8_t* bytes, size_t n, long long frame, Info* info, void* record, size_t capacity, size_t* needed, char* msg,
          size_t msg_cap);

// The header half of parse() alone: walks bytes[0, n) up to and including the SOS header and applies every rule parse() applies
// there (n need not reach the entropy-coded data). kOk: parse() would go on to decode the scan of this variant.
int probe(const uint8_t* bytes, size_t n, long long frame, Info* info, char* msg, size_t msg_cap);

// ---- the GPU entropy route (csrc/jpeg_entropy.hip): the host only walks the header and removes the byte stuffing
//
// Plan (little endian, 4-byte aligned):
//   PlanHeader                         112 bytes
//   uint16 quant[3][64]                as the record carries them
//   PlanHuff huff[6]                   the scan's tables by component: huff[c] decodes component c's DC symbols, huff[3 + c] its AC
//                                      symbols (a component the frame does not have: zeros)
//   uint8  stream[stream_bytes]        the entropy-coded segment with the stuffing removed (FF 00 -> FF), ended where the parser's
//                                      bit reader stops: the first FF that no 00 follows, or the end of the data; zeros up to a
//                                      multiple of 4 follow
constexpr uint32_t kPlanMagic = 0x3150474au;  // "JGP1"
constexpr int kHostRoute = 2;                 // plan(): a frame the GPU route does not take (restart intervals); parse() decodes it

struct PlanHuff {
  uint16_t look[512];                        // 9 leading bits -> (length << 8 | symbol), 0 = longer than 9 bits or no code
  int32_t maxcode[18];                       // [l], l = 1..16: largest code of length l, -1 if none
  int32_t valoff[18];                        // [l]: vals index of the first code of length l, minus that code
  uint8_t vals[256];
  uint32_t nvals, reserved;
};
static_assert(sizeof(PlanHuff) == 1432, "plan table layout");

struct PlanHeader {
  uint32_t magic, bytes;                     // bytes: the whole plan
  uint32_t width, height, ncomp, hs, vs, mcus_x, mcus_y, n_blocks;
  uint32_t bw[3], bh[3];
  uint32_t restart;                          // the restart interval: 0 in every plan plan() writes
  uint32_t td[3], ta[3];                     // the SOS header's table selectors, by component
  uint32_t stream_bytes, reserved;           // reserved: 0 in a plan; the number of intervals in an interval plan (below)
  uint64_t stream_bits;                      // bits of the clean stream: 8 * stream_bytes
};
static_assert(sizeof(PlanHeader) == 112, "plan header layout");
constexpr size_t kPlanQuantOffset = sizeof(PlanHeader);
constexpr size_t kPlanHuffOffset = kPlanQuantOffset + 3 * 64 * sizeof(uint16_t);
constexpr size_t kPlanStreamOffset = kPlanHuffOffset + 6 * sizeof(PlanHuff);
static_assert(kPlanStreamOffset % 16 == 0, "the stream starts 16-byte aligned");

// Most bits one block can take in any baseline scan: 64 symbols of a 16-bit code and a 15-bit amplitude.
constexpr size_t kMaxBlockBits = 64 * 31;
// Largest plan a decodable frame of h x w can need (every block kMaxBlockBits long, a padded last byte).
size_t plan_bound(int h, int w);

// The header half of parse() and the unstuffing: bytes[0, n) -> the plan in out[0, capacity) (4-byte aligned; may be NULL with
// capacity 0). Every refusal parse() makes up to and including the SOS header is made here with the same message. Returns kOk
// (plan written), kTooSmall (not written: call again with *needed bytes), kHostRoute (a restart interval: *needed is 0, nothing
// is written, *info is filled), kUnsupported or kInvalid. No byte outside bytes[0, n) is read, none outside out[0, capacity) written.
int plan(const uint8_t* bytes, size_t n, long long frame, Info* info, void* out, size_t capacity, size_t* needed, char* msg, size_t msg_cap);

// What the entropy kernels rely on in a plan: its sizes consistent with each other and with its length, a geometry parse() would
// have produced, no restart interval. (The tables are not trusted: the kernels bound every look-up themselves.) kOk or kInvalid.
int check_plan(const void* plan, size_t bytes, char* msg, size_t msg_cap);

// ---- the restart-interval route (csrc/jpeg_restart.hip): a frame with a DRI segment, one lane per restart interval
//
// At every RSTn the stream is byte aligned, the DC predictors are zero and the MCU index is known, so every interval decodes on
// its own. The host walks the header, removes the byte stuffing and the RSTn markers and notes where every interval starts.
//
// Interval plan (little endian, 4-byte aligned):
//   PlanHeader                         magic kIntervalPlanMagic, restart = Ri (MCUs per interval, > 0), reserved = n_intervals;
//                                      stream_bytes, stream_bits of the whole clean stream
//   uint16 quant[3][64], PlanHuff huff[6]   as in the plan above
//   uint32 start[n_intervals + 1]      byte offset of every interval in the clean stream; start[n_intervals] = stream_bytes.
//                                      n_intervals = ceil(mcus_x * mcus_y / Ri)
//   zeros up to a multiple of 16
//   uint8  stream[stream_bytes]        the intervals back to back: stuffing removed, markers and their fill bytes removed;
//                                      zeros up to a multiple of 4 follow
constexpr uint32_t kIntervalPlanMagic = 0x3249474au;   // "JGI2": check_plan() refuses it, check_plan_intervals() refuses a "JGP1"
constexpr int kNoRestart = 3;                 // plan_intervals(): the frame has no restart interval; nothing is written

inline size_t interval_count(size_t n_mcus, size_t restart) { return restart ? (n_mcus + restart - 1) / restart : 0; }
// Offset of the clean stream in an interval plan of n_intervals intervals (16-byte aligned).
inline size_t interval_stream_offset(size_t n_intervals) { return (kPlanStreamOffset + 4 * (n_intervals + 1) + 15) / 16 * 16; }
// Largest interval plan a decodable frame of h x w can need (one interval per MCU, every block kMaxBlockBits long and every
// interval's last byte padded).
size_t plan_intervals_bound(int h, int w);

// plan() for a frame that has a restart interval. The header walk and every refusal up to and including the SOS header are
// parse()'s, with the same status and message. The entropy-coded segment is then walked with memchr: an interval ends at the
// first FF that no 00 follows, where RSTn (after any FF fill bytes) must stand in sequence, RST7 followed by RST0; the last
// interval ends at the first marker or with the data, as the parser's bit reader does. Where a marker is missing, out of
// sequence or the data ends early, the Huffman decode of parse() runs to word the refusal: the status and message are
// parse()'s by construction. Returns kOk (plan written), kTooSmall (not written: call again with *needed bytes), kNoRestart
// (*needed is 0, nothing is written, *info is filled), kUnsupported or kInvalid. No byte outside bytes[0, n) is read, none
// outside out[0, capacity) written.
int plan_intervals(const uint8_t* bytes, size_t n, long long frame, Info* info, void* out, size_t capacity, size_t* needed, char* msg, size_t msg_cap);

// What the restart kernel relies on in an interval plan: the geometry rules of check_plan(), restart in 1..65535,
// n_intervals = ceil(n_mcus / restart), start[0] = 0, start[] monotone, start[n_intervals] = stream_bytes, and sizes that add up
// to the length. (The tables are not trusted: the kernel bounds every look-up itself.) kOk or kInvalid.
int check_plan_intervals(const void* plan, size_t bytes, char* msg, size_t msg_cap);

// What the device code relies on: sizes consistent with each other and with h x w, offsets monotone, every block at most 64
// long, the closing offset equal to the stream length, the record exactly `bytes` long. kOk or kInvalid with a message.
int check_record(const void* record, size_t bytes, int h, int w, char* msg, size_t msg_cap);

}  // namespace jpeg
}  // namespace gtx
