// Record -> baseline JFIF JPEG (jpeg_emit.hpp). The writer counts every byte and stores only those that fit, so a short buffer
// yields the size and nothing else; every index into the record comes from offsets that check_record has verified.
#include "jpeg_emit.hpp"

#include <cstdio>
#include <cstring>

#include "jpeg_std_huff.hpp"

namespace gtx {
namespace jpeg {
namespace {

// zigzag position -> natural (row-major) position
constexpr uint8_t kNatural[64] = {0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48,
                                  41, 34, 27, 20, 13, 6,  7,  14, 21, 28, 35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23,
                                  30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// ITU T.81 Annex K.1 / K.2, natural order
constexpr uint8_t kStdLumaQuant[64] = {16, 11, 10, 16, 24,  40,  51,  61,  12, 12, 14, 19, 26,  58,  60,  55,  14, 13, 16, 24, 40,  57,
                                       69, 56, 14, 17, 22,  29,  51,  87,  80, 62, 18, 22, 37,  56,  68,  109, 103, 77, 24, 35, 55,  64,
                                       81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr uint8_t kStdChromaQuant[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99,
                                         99, 99, 47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                         99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};

// symbol -> (code, length) of one Annex K.3 table; length 0: the table has no code for the symbol
struct EncTable {
  uint16_t code[256];
  uint8_t size[256];
  void build(const uint8_t bits[16], const uint8_t* vals) {
    memset(code, 0, sizeof code);
    memset(size, 0, sizeof size);
    unsigned c = 0;
    int k = 0;
    for (int l = 1; l <= 16; ++l) {
      for (int i = 0; i < bits[l - 1]; ++i, ++k, ++c) code[vals[k]] = (uint16_t)c, size[vals[k]] = (uint8_t)l;
      c <<= 1;
    }
  }
};

struct Tables {
  EncTable dc[2], ac[2];
  Tables() {
    dc[0].build(kStdDcLumaBits, kStdDcLumaVals);
    dc[1].build(kStdDcChromaBits, kStdDcChromaVals);
    ac[0].build(kStdAcLumaBits, kStdAcLumaVals);
    ac[1].build(kStdAcChromaBits, kStdAcChromaVals);
  }
};

// Counts every byte, stores those below `cap`.
struct Writer {
  uint8_t* out;
  size_t cap, n = 0;
  uint64_t acc = 0;            // the low `fill` bits are pending, oldest highest
  int fill = 0;

  void byte(unsigned b) {
    if (n < cap) out[n] = (uint8_t)b;
    ++n;
  }
  void u16(unsigned v) { byte(v >> 8), byte(v & 255); }
  void raw(const void* p, size_t k) {
    for (size_t i = 0; i < k; ++i) byte(static_cast<const uint8_t*>(p)[i]);
  }
  void bits(unsigned v, int k) {                                  // k <= 26
    acc = (acc << k) | (v & ((1u << k) - 1u));
    fill += k;
    while (fill >= 8) {
      const unsigned b = (unsigned)(acc >> (fill - 8)) & 255u;
      byte(b);
      if (b == 0xFF) byte(0);                                     // a stuffed FF
      fill -= 8;
    }
  }
  void flush() {                                                  // the last byte is padded with 1-bits
    if (fill) bits(0x7F, 8 - fill);
    acc = 0, fill = 0;
  }
};

inline int bit_length(unsigned v) { return v ? 32 - __builtin_clz(v) : 0; }

void dht(Writer& w, int cls_id, const uint8_t bits[16], const uint8_t* vals, int nvals) {
  w.byte((unsigned)cls_id);
  w.raw(bits, 16);
  w.raw(vals, (size_t)nvals);
}

// SOI, APP0, DQT, SOF0, DHT, SOS: everything in front of the scan (jpeg_emit.hpp: header())
// restart > 0: a DRI segment in front of SOS
void write_header(Writer& w, const RecordHeader& hd, const uint16_t* quant, unsigned restart = 0) {
  const int ncomp = (int)hd.ncomp;
  // Cr shares Cb's table when the two are equal (what libjpeg writes), else it gets a third
  const bool third = ncomp == 3 && memcmp(quant + 64, quant + 128, 128) != 0;
  const int n_tables = ncomp == 1 ? 1 : third ? 3 : 2;
  w.u16(0xFFD8);
  static const uint8_t app0[] = {0xFF, 0xE0, 0, 16, 'J', 'F', 'I', 'F', 0, 1, 1, 0, 0, 1, 0, 1, 0, 0};
  w.raw(app0, sizeof app0);
  for (int t = 0; t < n_tables; ++t) {
    w.u16(0xFFDB), w.u16(67), w.byte((unsigned)t);
    for (int z = 0; z < 64; ++z) w.byte(quant[64 * t + kNatural[z]]);
  }
  w.u16(0xFFC0), w.u16(8 + 3 * (unsigned)ncomp), w.byte(8), w.u16(hd.height), w.u16(hd.width), w.byte((unsigned)ncomp);
  for (int c = 0; c < ncomp; ++c) {
    w.byte((unsigned)c + 1);
    w.byte(c == 0 ? (hd.hs << 4 | hd.vs) : 0x11);
    w.byte(c == 0 ? 0u : (c == 2 && third) ? 2u : 1u);
  }
  const int n_huff = ncomp == 1 ? 1 : 2;
  w.u16(0xFFC4);
  w.u16(2 + (unsigned)n_huff * (17 + 12) + 17 + 162 + (n_huff == 2 ? 17 + 162 : 0));
  dht(w, 0x00, kStdDcLumaBits, kStdDcLumaVals, 12);
  dht(w, 0x10, kStdAcLumaBits, kStdAcLumaVals, 162);
  if (n_huff == 2) {
    dht(w, 0x01, kStdDcChromaBits, kStdDcChromaVals, 12);
    dht(w, 0x11, kStdAcChromaBits, kStdAcChromaVals, 162);
  }
  if (restart) w.u16(0xFFDD), w.u16(4), w.u16(restart);
  w.u16(0xFFDA), w.u16(6 + 2 * (unsigned)ncomp), w.byte((unsigned)ncomp);
  for (int c = 0; c < ncomp; ++c) w.byte((unsigned)c + 1), w.byte(c == 0 ? 0x00 : 0x11);
  w.byte(0), w.byte(63), w.byte(0);
}

}  // namespace

bool quality_tables(int quality, uint16_t luma[64], uint16_t chroma[64]) {
  if (quality < 1 || quality > 100) return false;
  const int scale = quality < 50 ? 5000 / quality : 200 - 2 * quality;
  for (int i = 0; i < 64; ++i) {
    const int l = (kStdLumaQuant[i] * scale + 50) / 100, c = (kStdChromaQuant[i] * scale + 50) / 100;
    luma[i] = (uint16_t)(l < 1 ? 1 : l > 255 ? 255 : l);
    chroma[i] = (uint16_t)(c < 1 ? 1 : c > 255 ? 255 : c);
  }
  return true;
}

bool make_header(int h, int w, int ncomp, int hs, int vs, RecordHeader* hd) {
  if (h <= 0 || w <= 0 || h > kMaxDim || w > kMaxDim || !hd) return false;
  const bool samp = ncomp == 1 ? (hs == 1 && vs == 1) : ncomp == 3 && ((hs == 1 && vs == 1) || (hs == 2 && vs == 1) || (hs == 2 && vs == 2));
  if (!samp) return false;
  memset(hd, 0, sizeof *hd);
  hd->magic = kMagic;
  hd->width = (uint32_t)w, hd->height = (uint32_t)h, hd->ncomp = (uint32_t)ncomp, hd->hs = (uint32_t)hs, hd->vs = (uint32_t)vs;
  hd->mcus_x = (uint32_t)((w + 8 * hs - 1) / (8 * hs)), hd->mcus_y = (uint32_t)((h + 8 * vs - 1) / (8 * vs));
  hd->n_blocks = hd->mcus_x * hd->mcus_y * (uint32_t)(ncomp == 1 ? 1 : hs * vs + 2);
  hd->bw[0] = hd->mcus_x * (uint32_t)hs, hd->bh[0] = hd->mcus_y * (uint32_t)vs;
  for (int c = 1; c < ncomp; ++c) hd->bw[c] = hd->mcus_x, hd->bh[c] = hd->mcus_y;
  return true;
}

size_t header(const RecordHeader& hd, const uint16_t* quant, uint8_t* out, size_t capacity) {
  Writer w{out, out ? capacity : 0};
  write_header(w, hd, quant);
  return w.n;
}

void std_huff_codes(HuffCodes* out) {
  const Tables t;
  for (int k = 0; k < 2; ++k) {
    for (int s = 0; s < 12; ++s) out->dc[k][s] = (uint32_t)t.dc[k].code[s] | (uint32_t)t.dc[k].size[s] << 16;
    for (int s = 0; s < 256; ++s) out->ac[k][s] = (uint32_t)t.ac[k].code[s] | (uint32_t)t.ac[k].size[s] << 16;
  }
}

int emit(const void* record, size_t bytes, uint8_t* out, size_t capacity, size_t* n, char* msg, size_t msg_cap) {
  return emit_restart(record, bytes, 0, out, capacity, n, msg, msg_cap);
}

int emit_restart(const void* record, size_t bytes, unsigned restart_mcus, uint8_t* out, size_t capacity, size_t* n, char* msg, size_t msg_cap) {
  static const Tables tables;
  if (msg && msg_cap) msg[0] = 0;
  if (n) *n = 0;
  auto bad = [&](const char* what) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "JPEG record: %s", what);
    return kInvalid;
  };
  if (restart_mcus > 65535u) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "JPEG emit: a restart interval of %u MCUs (DRI holds 0..65535)", restart_mcus);
    return kInvalid;
  }
  if (!record || bytes < sizeof(RecordHeader)) return bad("too short or misaligned");
  if (!out && capacity) return bad("no output buffer for the capacity given");
  RecordHeader hd;
  memcpy(&hd, record, sizeof hd);
  if (hd.width > (uint32_t)kMaxDim || hd.height > (uint32_t)kMaxDim) return bad("its frame size differs from h x w");
  if (check_record(record, bytes, (int)hd.height, (int)hd.width, msg, msg_cap) != kOk) return kInvalid;
  const uint8_t* rec = static_cast<const uint8_t*>(record);
  const uint16_t* quant = reinterpret_cast<const uint16_t*>(rec + kQuantOffset);
  const uint32_t* off = reinterpret_cast<const uint32_t*>(rec + kOffsetsOffset);
  const int16_t* coef = reinterpret_cast<const int16_t*>(rec + kOffsetsOffset + 4 * ((size_t)hd.n_blocks + 1));
  const int ncomp = (int)hd.ncomp;
  for (int i = 0; i < 64 * ncomp; ++i)
    if (quant[i] > 255) return bad("a quantiser above 255 (baseline tables have 8-bit entries)");

  Writer w{out, out ? capacity : 0};
  write_header(w, hd, quant, restart_mcus);

  const uint32_t luma = hd.hs * hd.vs, bpm = ncomp == 1 ? 1u : luma + 2u;
  int pred[3] = {0, 0, 0};
  uint32_t k = 0;                                                  // position inside the MCU
  uint32_t mcu = 0;
  unsigned next_rst = 0;
  for (uint32_t b = 0; b < hd.n_blocks; ++b) {
    if (restart_mcus && k == 0 && mcu && mcu % restart_mcus == 0) {   // the interval's last byte padded with 1-bits, RSTn, predictors reset
      w.flush();
      w.u16(0xFFD0 + next_rst);
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
    }
    const int c = (ncomp == 1 || k < luma) ? 0 : 1 + (int)(k - luma);
    const EncTable &td = tables.dc[c ? 1 : 0], &ta = tables.ac[c ? 1 : 0];
    const int16_t* v = coef + off[b];
    const int len = (int)(off[b + 1] - off[b]);                   // 0..64, inside the stream: check_record
    const int dcv = len ? v[0] : 0, diff = dcv - pred[c];
    pred[c] = dcv;
    unsigned mag = (unsigned)(diff < 0 ? -diff : diff);
    int s = bit_length(mag);
    if (s > 11) return bad("a DC difference beyond 11 bits (no Annex K.3 code)");
    w.bits(td.code[s], td.size[s]);
    if (s) w.bits((unsigned)(diff < 0 ? diff - 1 : diff), s);
    int run = 0;
    for (int z = 1; z < len; ++z) {
      const int a = v[z];
      if (a == 0) {
        ++run;
        continue;
      }
      for (; run > 15; run -= 16) w.bits(ta.code[0xF0], ta.size[0xF0]);
      mag = (unsigned)(a < 0 ? -a : a);
      s = bit_length(mag);
      if (s > 10) return bad("an AC coefficient beyond 10 bits (no Annex K.3 code)");
      const int sym = run << 4 | s;
      w.bits(ta.code[sym], ta.size[sym]);
      w.bits((unsigned)(a < 0 ? a - 1 : a), s);
      run = 0;
    }
    // zeros up to position 63 follow (a run that ends in a zero inside the record counts among them): end of block
    int last = len;
    while (last > 1 && v[last - 1] == 0) --last;
    if (last < 64) w.bits(ta.code[0], ta.size[0]);
    if (++k == bpm) k = 0, ++mcu;
  }
  w.flush();
  w.u16(0xFFD9);
  if (n) *n = w.n;
  return w.n <= w.cap ? kOk : kTooSmall;
}

}  // namespace jpeg
}  // namespace gtx
