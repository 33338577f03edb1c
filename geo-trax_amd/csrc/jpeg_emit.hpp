// Host half of the JPEG frame sink: the packed record of jpeg_parse.hpp (from the GPU encoder, csrc/jpeg_enc.hip, or from the
// parser) -> one baseline JFIF JPEG. It replaces the entropy-coding half of cv2.VideoWriter.write() (geotrax/visualize.py:298);
// colour conversion, chroma downsampling, the forward DCT and quantisation are csrc/jpeg_enc.hip's. Plain C++, no HIP: it
// compiles alone (csrc/diag/jpeg_emit_check.cpp runs it under the sanitizers).
#pragma once
#include <cstddef>
#include <cstdint>

#include "jpeg_parse.hpp"

namespace gtx {
namespace jpeg {

// jpeg_set_quality(quality, force_baseline = TRUE): jpeg_quality_scaling applied to the ITU T.81 Annex K.1 / K.2 tables, clamped
// to 1..255; natural (row-major) order. quality outside 1..100: false, nothing written.
bool quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64]);

// The header of the record a w x h frame of `ncomp` components with luma sampling hs x vs has (everything but n_coef and bytes,
// which depend on the data). false: a size or a sampling outside the accepted set.
bool make_header(int h, int w, int ncomp, int hs, int vs, RecordHeader* hd);

// Writes the record (`bytes` long, 4-byte aligned; check_record runs first) as a baseline JFIF file into out[0, capacity):
// SOI, APP0, DQT, SOF0, DHT (the Annex K.3 tables), SOS, the Huffman-coded scan with FF bytes stuffed, EOI. *n receives the
// file's size whenever the record can be coded. Returns kOk (written), kTooSmall (capacity < *n: call again with *n bytes;
// nothing outside out[0, capacity) was touched) or kInvalid with a message: a damaged record, a quantiser above 255, or a
// coefficient the Annex K.3 tables have no code for (a DC difference beyond 11 bits, an AC value beyond 10: no 8-bit picture
// yields one). Every record the parser produces from 8-bit pictures is accepted: grayscale, 4:4:4, 4:2:2, 4:2:0.
int emit(const void* record, size_t bytes, uint8_t* out, size_t capacity, size_t* n, char* msg, size_t msg_cap);

// emit() with restart intervals of `restart_mcus` MCUs, so that the file decodes one lane per interval (csrc/jpeg_restart.hip): a
// DRI segment in front of SOS and, before every MCU whose index is a multiple of restart_mcus (but the first), the pending byte
// padded with 1-bits, RSTn (n counts 0..7 and wraps) and the DC predictors back at 0. restart_mcus = 0: emit()'s bytes exactly.
// Above 65535 (what DRI holds): kInvalid. Everything else as emit().
int emit_restart(const void* record, size_t bytes, unsigned restart_mcus, uint8_t* out, size_t capacity, size_t* n, char* msg, size_t msg_cap);

// The picture's header alone, the bytes emit() writes in front of the scan: SOI, APP0, DQT (one table per component; Cr shares
// Cb's when the two are equal), SOF0, DHT, SOS. It depends on the frame's size, sampling and quantisers only (hd's width, height,
// ncomp, hs, vs; quant[3][64] in natural order), so both entropy routes call it: emit() per picture, the GPU coder
// (csrc/jpeg_huff.hip) once per encoder. Returns the header's length and stores the bytes below `capacity`.
constexpr size_t kMaxHeaderBytes = 704;       // 2 + 18 + 3 * 69 + 19 + 420 + 14 = 680 for three components and three tables
size_t header(const RecordHeader& hd, const uint16_t* quant, uint8_t* out, size_t capacity);

// The Annex K.3 tables as the encoder reads them: entry = code | length << 16. dc[t][category 0..11], ac[t][run << 4 | size];
// t = 0 luma, 1 chroma. An entry of 0: the table has no code for the symbol.
struct HuffCodes {
  uint32_t dc[2][12];
  uint32_t ac[2][256];
};
void std_huff_codes(HuffCodes* out);

}  // namespace jpeg
}  // namespace gtx
