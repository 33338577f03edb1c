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

// What the device code relies on: sizes consistent with each other and with h x w, offsets monotone, every block at most 64
// long, the closing offset equal to the stream length, the record exactly `bytes` long. kOk or kInvalid with a message.
int check_record(const void* record, size_t bytes, int h, int w, char* msg, size_t msg_cap);

}  // namespace jpeg
}  // namespace gtx
