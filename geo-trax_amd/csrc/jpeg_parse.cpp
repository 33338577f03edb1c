// Baseline JPEG marker walk + Huffman decode into the packed record of jpeg_parse.hpp. Every length and every code length
// comes from the file and is checked against the buffer before it is used.
#include "jpeg_parse.hpp"

#include <cstdarg>
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

struct Failure {
  int code;
};

struct Huff {
  bool defined = false;
  uint8_t vals[256];
  int nvals = 0;
  int32_t maxcode[17];         // largest code of length l, -1 if none
  int32_t valoff[17];          // vals index of the first code of length l, minus that code
  uint16_t look[512];          // 9 leading bits -> (length << 8 | symbol), 0 = longer than 9 bits or no code

  // bits[l - 1] = number of codes of length l. false: the counts do not describe a prefix code
  bool build(const uint8_t* bits, const uint8_t* v, int n) {
    memcpy(vals, v, (size_t)n);
    nvals = n;
    memset(look, 0, sizeof look);
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
      valoff[l] = k - code;
      const int cnt = bits[l - 1];
      if (code + cnt > (1 << l)) return false;
      for (int i = 0; i < cnt; ++i, ++k, ++code) {
        if (l <= 9) {
          const int first = code << (9 - l);
          for (int j = 0; j < (1 << (9 - l)); ++j) look[first + j] = (uint16_t)((l << 8) | vals[k]);
        }
      }
      maxcode[l] = cnt ? code - 1 : -1;
      code <<= 1;
    }
    defined = true;
    return true;
  }
};

struct Parser {
  const uint8_t* p = nullptr;
  size_t n = 0;
  long long frame = 0;
  char* msg = nullptr;
  size_t msg_cap = 0;

  [[noreturn]] void fail(int code, const char* fmt, ...) {
    if (msg && msg_cap) {
      const int k = snprintf(msg, msg_cap, "JPEG frame %lld: ", frame);
      if (k > 0 && (size_t)k < msg_cap) {
        va_list ap;
        va_start(ap, fmt);
        vsnprintf(msg + k, msg_cap - (size_t)k, fmt, ap);
        va_end(ap);
      }
    }
    throw Failure{code};
  }

  // ---- header state
  bool have_sof = false, any_dht = false, jfif = false;
  int width = 0, height = 0, ncomp = 0, hs = 1, vs = 1, restart = 0, adobe = -1;
  int comp_id[3] = {0, 0, 0}, comp_tq[3] = {0, 0, 0}, scan_td[3] = {0, 0, 0}, scan_ta[3] = {0, 0, 0};
  bool have_q[4] = {false, false, false, false};
  uint16_t quant[4][64];
  Huff dc[4], ac[4];

  uint8_t u8(size_t pos) {
    if (pos >= n) fail(kInvalid, "the data ends inside a segment (byte %zu)", pos);
    return p[pos];
  }
  unsigned u16(size_t pos) { return ((unsigned)u8(pos) << 8) | u8(pos + 1); }

  // ---- entropy-coded segment
  size_t pos = 0;
  uint64_t acc = 0;            // left-aligned: the top `avail` bits are the next bits of the stream
  int avail = 0;
  bool stopped = false;        // a marker or the end of the buffer: no more bits to fetch

  void fill() {
    while (avail <= 56 && !stopped) {
      if (pos >= n) { stopped = true; break; }
      const uint8_t b = p[pos];
      if (b == 0xFF) {
        if (pos + 1 >= n || p[pos + 1] != 0) { stopped = true; break; }
        pos += 2;              // FF 00: a stuffed FF
      } else {
        pos += 1;
      }
      acc |= (uint64_t)b << (56 - avail);
      avail += 8;
    }
  }
  void consume(int k) {
    if (k > avail) fail(kInvalid, "the entropy-coded data ends early (byte %zu of %zu)", pos, n);
    acc <<= k;
    avail -= k;
  }
  int decode(const Huff& t) {
    if (avail < 32) fill();
    const unsigned top = (unsigned)(acc >> 48);                   // 16 bits, zero-padded past the end of the data
    const unsigned e = t.look[top >> 7];
    if (e) {
      consume((int)(e >> 8));
      return (int)(e & 255);
    }
    for (int l = 10; l <= 16; ++l) {
      const int code = (int)(top >> (16 - l));
      if (code <= t.maxcode[l]) {
        const int idx = t.valoff[l] + code;
        if (idx < 0 || idx >= t.nvals) break;
        consume(l);
        return t.vals[idx];
      }
    }
    fail(kInvalid, "a Huffman code that is in no table (byte %zu)", pos);
  }
  int receive_extend(int s) {                                     // s in 1..15
    const int v = (int)(acc >> (64 - s));
    consume(s);
    return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v;
  }

  void segments(Info* info);
  void sof(unsigned m, size_t at, size_t len, Info* info);
  void geometry(RecordHeader* hd) const;
  int scan(void* record, size_t capacity, size_t* needed);
  int write_plan(void* out, size_t capacity, size_t* needed);
  void write_plan_head(uint8_t* dst, uint32_t magic, size_t total, size_t len, uint32_t n_intervals) const;
  int write_interval_plan(void* out, size_t capacity, size_t* needed);
};

const char* sof_name(unsigned m) {
  switch (m) {
    case 0xC1: return "SOF1 (extended sequential)";
    case 0xC2: return "SOF2 (progressive)";
    case 0xC3: return "SOF3 (lossless)";
    case 0xC5: return "SOF5 (differential sequential)";
    case 0xC6: return "SOF6 (differential progressive)";
    case 0xC7: return "SOF7 (differential lossless)";
    case 0xC9: return "SOF9 (arithmetic coding)";
    case 0xCA: return "SOF10 (progressive, arithmetic coding)";
    case 0xCB: return "SOF11 (lossless, arithmetic coding)";
    case 0xCD: return "SOF13 (differential, arithmetic coding)";
    case 0xCE: return "SOF14 (differential progressive, arithmetic coding)";
    case 0xCF: return "SOF15 (differential lossless, arithmetic coding)";
  }
  return "SOF";
}

void Parser::sof(unsigned m, size_t at, size_t len, Info* info) {
  if (m != 0xC0) fail(kUnsupported, "%s is not decoded (baseline SOF0 only)", sof_name(m));
  if (have_sof) fail(kInvalid, "a second SOF0 segment");
  if (len < 8) fail(kInvalid, "SOF0 segment of %zu bytes", len);
  const int prec = u8(at), nf = u8(at + 5);
  height = (int)u16(at + 1), width = (int)u16(at + 3);
  if (prec != 8) fail(kUnsupported, "SOF0 with %d-bit samples (8-bit only)", prec);
  if (nf == 4) fail(kUnsupported, "SOF0 with four components (CMYK / YCCK)");
  if (nf != 1 && nf != 3) fail(kUnsupported, "SOF0 with %d components", nf);
  if (len != (size_t)(8 + 3 * nf)) fail(kInvalid, "SOF0 segment of %zu bytes for %d components", len, nf);
  if (width <= 0 || height <= 0) fail(kInvalid, "SOF0 with a %d x %d frame", width, height);
  if (width > kMaxDim || height > kMaxDim) fail(kUnsupported, "SOF0 with a %d x %d frame (larger than %d)", width, height, kMaxDim);
  int h[3], v[3];
  for (int c = 0; c < nf; ++c) {
    comp_id[c] = u8(at + 6 + 3 * c);
    h[c] = u8(at + 7 + 3 * c) >> 4, v[c] = u8(at + 7 + 3 * c) & 15;
    comp_tq[c] = u8(at + 8 + 3 * c);
    if (h[c] < 1 || h[c] > 4 || v[c] < 1 || v[c] > 4) fail(kInvalid, "SOF0 with sampling factors %d x %d", h[c], v[c]);
    if (comp_tq[c] > 3) fail(kInvalid, "SOF0 names quantisation table %d", comp_tq[c]);
  }
  ncomp = nf, hs = 1, vs = 1;                                     // one component: a non-interleaved scan, its factors do not matter
  if (nf == 3) {
    const bool ok = h[1] == 1 && v[1] == 1 && h[2] == 1 && v[2] == 1 && ((h[0] == 1 && v[0] == 1) || (h[0] == 2 && v[0] == 1) || (h[0] == 2 && v[0] == 2));
    if (!ok)
      fail(kUnsupported, "SOF0 with sampling %dx%d,%dx%d,%dx%d (4:4:4, 4:2:2 and 4:2:0 only)", h[0], v[0], h[1], v[1], h[2], v[2]);
    hs = h[0], vs = v[0];
  }
  have_sof = true;
  if (info) info->width = width, info->height = height, info->ncomp = ncomp, info->hs = hs, info->vs = vs;
}

// Walks the segments up to and including the SOS header; pos is left at the first entropy-coded byte.
void Parser::segments(Info* info) {
  if (n < 4 || p[0] != 0xFF || p[1] != 0xD8) fail(kInvalid, "no SOI marker at the start");
  size_t at = 2;
  for (;;) {
    if (u8(at) != 0xFF) fail(kInvalid, "byte %zu should start a marker", at);
    while (u8(at) == 0xFF) ++at;                                  // fill bytes
    const unsigned m = p[at++];
    if (m == 0xD9) fail(kInvalid, "EOI before any scan");
    if (m == 0x00 || m == 0x01 || (m >= 0xD0 && m <= 0xD8)) fail(kInvalid, "marker FF%02X between segments", m);
    const size_t len = u16(at);                                   // counts its own two bytes
    if (len < 2 || at + len > n) fail(kInvalid, "segment FF%02X of %zu bytes at byte %zu runs past the data", m, len, at);
    const size_t body = at + 2, end = at + len;
    if (m == 0xC4) {                                              // DHT
      for (size_t q = body; q < end;) {
        if (q + 17 > end) fail(kInvalid, "DHT segment is cut short");
        const int tc = p[q] >> 4, th = p[q] & 15;
        int total = 0;
        for (int i = 0; i < 16; ++i) total += p[q + 1 + i];
        if (tc > 1 || th > 3) fail(kInvalid, "DHT names table class %d id %d", tc, th);
        if (total > 256 || q + 17 + (size_t)total > end) fail(kInvalid, "DHT table with %d codes does not fit its segment", total);
        if (!(tc ? ac : dc)[th].build(p + q + 1, p + q + 17, total)) fail(kInvalid, "DHT code lengths are not a prefix code");
        any_dht = true;
        q += 17 + (size_t)total;
      }
    } else if (m == 0xDB) {                                       // DQT
      for (size_t q = body; q < end;) {
        const int pq = p[q] >> 4, tq = p[q] & 15;
        if (pq == 1) fail(kUnsupported, "DQT with 16-bit entries (8-bit tables only)");
        if (pq != 0 || tq > 3) fail(kInvalid, "DQT names precision %d table %d", pq, tq);
        if (q + 65 > end) fail(kInvalid, "DQT segment is cut short");
        for (int k = 0; k < 64; ++k) quant[tq][kNatural[k]] = p[q + 1 + k];
        have_q[tq] = true;
        q += 65;
      }
    } else if (m == 0xDD) {                                       // DRI
      if (len != 4) fail(kInvalid, "DRI segment of %zu bytes", len);
      restart = (int)u16(body);
    } else if (m == 0xE0) {                                       // APP0: a JFIF header says the components are YCbCr
      if (len >= 7 && memcmp(p + body, "JFIF", 5) == 0) jfif = true;
    } else if (m == 0xEE) {                                       // APP14: Adobe's colour transform flag
      if (len >= 14 && memcmp(p + body, "Adobe", 5) == 0) adobe = p[body + 11];
    } else if (m == 0xC0 || (m >= 0xC1 && m <= 0xCF && m != 0xC8 && m != 0xCC)) {
      sof(m, body, len, info);
    } else if (m == 0xCC) {
      fail(kUnsupported, "DAC (arithmetic coding conditioning) is not decoded");
    } else if (m == 0xDA) {                                       // SOS
      if (!have_sof) fail(kInvalid, "SOS before SOF0");
      const int ns = u8(body);
      if (ns < 1 || ns > 4 || len != (size_t)(6 + 2 * ns)) fail(kInvalid, "SOS segment of %zu bytes for %d components", len, ns);
      if (ns != ncomp) fail(kUnsupported, "SOS with %d of %d components (non-interleaved multi-scan colour)", ns, ncomp);
      if (adobe == 2 || (adobe == 0 && ncomp == 3)) fail(kUnsupported, "APP14 Adobe transform %d (%s) is not decoded", adobe, adobe ? "YCCK" : "RGB");
      // libjpeg's guess without JFIF or Adobe markers: component ids 'R', 'G', 'B' mean RGB data, anything else YCbCr
      if (ncomp == 3 && !jfif && adobe < 0 && comp_id[0] == 'R' && comp_id[1] == 'G' && comp_id[2] == 'B')
        fail(kUnsupported, "SOF0 with component ids 'R', 'G', 'B' and no JFIF / Adobe marker (RGB data) is not decoded");
      if (!any_dht) {                                             // Motion-JPEG frames may leave the tables out: Annex K.3
        dc[0].build(kStdDcLumaBits, kStdDcLumaVals, (int)sizeof kStdDcLumaVals);
        dc[1].build(kStdDcChromaBits, kStdDcChromaVals, (int)sizeof kStdDcChromaVals);
        ac[0].build(kStdAcLumaBits, kStdAcLumaVals, (int)sizeof kStdAcLumaVals);
        ac[1].build(kStdAcChromaBits, kStdAcChromaVals, (int)sizeof kStdAcChromaVals);
      }
      for (int c = 0; c < ns; ++c) {
        const int id = p[body + 1 + 2 * c], td = p[body + 2 + 2 * c] >> 4, ta = p[body + 2 + 2 * c] & 15;
        if (id != comp_id[c]) fail(kInvalid, "SOS lists component %d where SOF0 has %d", id, comp_id[c]);
        if (td > 3 || ta > 3 || !dc[td].defined || !ac[ta].defined) fail(kInvalid, "SOS names Huffman tables %d / %d that no DHT defined", td, ta);
        if (!have_q[comp_tq[c]]) fail(kInvalid, "component %d uses quantisation table %d that no DQT defined", c, comp_tq[c]);
        scan_td[c] = td, scan_ta[c] = ta;
      }
      const size_t q = body + 1 + 2 * (size_t)ns;
      if (p[q] != 0 || p[q + 1] != 63 || p[q + 2] != 0) fail(kInvalid, "SOS with spectral selection %d..%d, approximation %02X in a baseline frame", p[q], p[q + 1], p[q + 2]);
      pos = end;
      return;
    }                                                             // APPn, COM and anything else with a length: skipped by it
    at = end;
  }
}

// The record header's geometry fields from the frame header (n_coef and bytes stay 0).
void Parser::geometry(RecordHeader* out) const {
  RecordHeader hd;
  memset(&hd, 0, sizeof hd);
  hd.magic = kMagic;
  hd.width = (uint32_t)width, hd.height = (uint32_t)height, hd.ncomp = (uint32_t)ncomp, hd.hs = (uint32_t)hs, hd.vs = (uint32_t)vs;
  hd.mcus_x = (uint32_t)((width + 8 * hs - 1) / (8 * hs)), hd.mcus_y = (uint32_t)((height + 8 * vs - 1) / (8 * vs));
  const int bpm = ncomp == 1 ? 1 : hs * vs + 2;
  hd.n_blocks = (uint32_t)((size_t)hd.mcus_x * hd.mcus_y * (size_t)bpm);
  hd.bw[0] = hd.mcus_x * (uint32_t)hs, hd.bh[0] = hd.mcus_y * (uint32_t)vs;
  for (int c = 1; c < ncomp; ++c) hd.bw[c] = hd.mcus_x, hd.bh[c] = hd.mcus_y;
  *out = hd;
}

// Decodes the scan into the record. Returns kOk or kTooSmall; *needed is the record's size either way.
int Parser::scan(void* record, size_t capacity, size_t* needed) {
  RecordHeader hd;
  geometry(&hd);
  const size_t n_mcu = (size_t)hd.mcus_x * hd.mcus_y, n_blocks = hd.n_blocks;

  uint8_t* rec = static_cast<uint8_t*>(record);
  const size_t coef_base = kOffsetsOffset + 4 * (n_blocks + 1);
  bool writing = rec != nullptr && capacity >= coef_base;        // the offsets fit; the stream is checked block by block
  uint32_t* offsets = writing ? reinterpret_cast<uint32_t*>(rec + kOffsetsOffset) : nullptr;
  int16_t* coefs = writing ? reinterpret_cast<int16_t*>(rec + coef_base) : nullptr;
  const size_t coef_cap = writing ? (capacity - coef_base) / 2 : 0;

  int comp_of[6], n_in_mcu = 0;
  if (ncomp == 1) {
    comp_of[n_in_mcu++] = 0;
  } else {
    for (int k = 0; k < hs * vs; ++k) comp_of[n_in_mcu++] = 0;
    comp_of[n_in_mcu++] = 1;
    comp_of[n_in_mcu++] = 2;
  }
  int pred[3] = {0, 0, 0};
  unsigned next_rst = 0;
  size_t n_coef = 0, b = 0;
  int16_t blk[64];
  acc = 0, avail = 0, stopped = false;
  for (size_t mcu = 0; mcu < n_mcu; ++mcu) {
    if (restart && mcu && mcu % (size_t)restart == 0) {
      // the interval's last byte is padded with 1-bits; whole bytes left over mean the marker is not where it belongs
      if (avail >= 8) fail(kInvalid, "restart marker RST%u is not where the interval ends (byte %zu)", next_rst, pos);
      acc = 0, avail = 0, stopped = false;
      if (pos + 1 >= n) fail(kInvalid, "the entropy-coded data ends early (restart marker RST%u missing)", next_rst);
      if (p[pos] != 0xFF) fail(kInvalid, "restart marker RST%u is not where the interval ends (byte %zu)", next_rst, pos);
      while (pos < n && p[pos] == 0xFF) ++pos;
      if (pos >= n) fail(kInvalid, "the entropy-coded data ends early (restart marker RST%u missing)", next_rst);
      if (p[pos] != 0xD0 + next_rst) fail(kInvalid, "restart markers out of sequence: FF%02X where RST%u belongs (byte %zu)", p[pos], next_rst, pos);
      ++pos;
      next_rst = (next_rst + 1) & 7;
      pred[0] = pred[1] = pred[2] = 0;
    }
    for (int k = 0; k < n_in_mcu; ++k, ++b) {
      const int c = comp_of[k];
      const Huff &td = dc[scan_td[c]], &ta = ac[scan_ta[c]];
      memset(blk, 0, sizeof blk);
      int s = decode(td);
      if (s > 15) fail(kInvalid, "DC category %d", s);
      if (s) {
        if (avail < 16) fill();
        pred[c] += receive_extend(s);
      }
      if (pred[c] < -32768 || pred[c] > 32767) fail(kInvalid, "DC value %d does not fit 16 bits", pred[c]);
      blk[0] = (int16_t)pred[c];
      int len = pred[c] ? 1 : 0;
      for (int z = 1; z < 64;) {
        const int rs = decode(ta), r = rs >> 4;
        s = rs & 15;
        if (s == 0) {
          if (r != 15) break;                                     // EOB
          z += 16;
          continue;
        }
        z += r;
        if (z > 63) fail(kInvalid, "a run of zeros leaves the block (coefficient %d)", z);
        if (avail < 16) fill();
        blk[z] = (int16_t)receive_extend(s);                      // s >= 1: never zero
        len = ++z;
      }
      if (writing && n_coef + (size_t)len > coef_cap) writing = false;
      if (writing) {
        offsets[b] = (uint32_t)n_coef;
        memcpy(coefs + n_coef, blk, (size_t)len * 2);
      }
      n_coef += (size_t)len;
    }
  }
  const size_t total = record_bytes(n_blocks, n_coef);
  if (needed) *needed = total;
  if (!writing) return kTooSmall;
  offsets[n_blocks] = (uint32_t)n_coef;
  hd.n_coef = (uint32_t)n_coef, hd.bytes = (uint32_t)total;
  memcpy(rec, &hd, sizeof hd);
  for (int c = 0; c < 3; ++c) memcpy(rec + kQuantOffset + 128 * (size_t)c, quant[comp_tq[c < ncomp ? c : 0]], 128);
  return kOk;
}

// The plan of jpeg_parse.hpp for the frame whose header segments() has walked; pos is at the first entropy-coded byte.
int Parser::write_plan(void* out, size_t capacity, size_t* needed) {
  uint8_t* dst = static_cast<uint8_t*>(out);
  // fill()'s walk over the segment, a run of plain bytes at a time: FF 00 is an FF, any other FF (or one the data ends on) ends it.
  // Once to measure, and only when the plan fits once more to copy: a plan that does not fit leaves `out` untouched.
  auto walk = [&](uint8_t* to) {
    size_t len = 0, at = pos;
    while (at < n) {
      const uint8_t* ff = static_cast<const uint8_t*>(memchr(p + at, 0xFF, n - at));
      const size_t run = ff ? (size_t)(ff - (p + at)) : n - at;
      if (to && run) memcpy(to + len, p + at, run);
      len += run, at += run;
      if (!ff || at + 1 >= n || p[at + 1] != 0) break;
      if (to) to[len] = 0xFF;
      len += 1, at += 2;
    }
    return len;
  };
  const size_t len = walk(nullptr);
  const size_t padded = (len + 3) / 4 * 4, total = kPlanStreamOffset + padded;
  if (needed) *needed = total;
  if (!dst || capacity < total) return kTooSmall;
  walk(dst + kPlanStreamOffset);
  memset(dst + kPlanStreamOffset + len, 0, padded - len);
  write_plan_head(dst, kPlanMagic, total, len, 0);
  return kOk;
}

// The header, quantisers and tables both plan formats share, for the frame whose header segments() has walked.
void Parser::write_plan_head(uint8_t* dst, uint32_t magic, size_t total, size_t len, uint32_t n_intervals) const {
  RecordHeader g;
  geometry(&g);
  PlanHeader ph;
  memset(&ph, 0, sizeof ph);
  ph.magic = magic, ph.bytes = (uint32_t)total;
  ph.width = g.width, ph.height = g.height, ph.ncomp = g.ncomp, ph.hs = g.hs, ph.vs = g.vs, ph.mcus_x = g.mcus_x, ph.mcus_y = g.mcus_y, ph.n_blocks = g.n_blocks;
  for (int c = 0; c < 3; ++c) ph.bw[c] = g.bw[c], ph.bh[c] = g.bh[c];
  ph.restart = (uint32_t)restart;
  for (int c = 0; c < ncomp; ++c) ph.td[c] = (uint32_t)scan_td[c], ph.ta[c] = (uint32_t)scan_ta[c];
  ph.stream_bytes = (uint32_t)len, ph.stream_bits = 8 * (uint64_t)len, ph.reserved = n_intervals;
  memcpy(dst, &ph, sizeof ph);
  for (int c = 0; c < 3; ++c) memcpy(dst + kPlanQuantOffset + 128 * (size_t)c, quant[comp_tq[c < ncomp ? c : 0]], 128);
  memset(dst + kPlanHuffOffset, 0, 6 * sizeof(PlanHuff));
  for (int c = 0; c < ncomp; ++c)
    for (int cls = 0; cls < 2; ++cls) {
      const Huff& t = cls ? ac[scan_ta[c]] : dc[scan_td[c]];
      PlanHuff h;
      memset(&h, 0, sizeof h);
      memcpy(h.look, t.look, sizeof h.look);
      for (int l = 1; l <= 16; ++l) h.maxcode[l] = t.maxcode[l], h.valoff[l] = t.valoff[l];
      h.maxcode[0] = h.maxcode[17] = -1;
      memcpy(h.vals, t.vals, (size_t)t.nvals);
      h.nvals = (uint32_t)t.nvals;
      memcpy(dst + kPlanHuffOffset + sizeof(PlanHuff) * (size_t)(3 * cls + c), &h, sizeof h);
    }
}

// The interval plan of jpeg_parse.hpp; pos is at the first entropy-coded byte and restart > 0.
int Parser::write_interval_plan(void* out, size_t capacity, size_t* needed) {
  uint8_t* dst = static_cast<uint8_t*>(out);
  RecordHeader g;
  geometry(&g);
  const size_t n_mcu = (size_t)g.mcus_x * g.mcus_y, n_int = interval_count(n_mcu, (size_t)restart), stream_at = interval_stream_offset(n_int);
  // One pass measures, and only when the plan fits a second one copies. An interval is fill()'s walk, a run of plain bytes at a
  // time: FF 00 is an FF, any other FF (or one the data ends on) ends it. Behind every interval but the last, scan()'s marker
  // rules: at least two bytes left, FF fill bytes, then RSTn in sequence. false: scan() refuses this frame at that marker or before.
  auto walk = [&](uint8_t* to, uint32_t* start, size_t* total) {
    size_t len = 0, at = pos;
    unsigned next_rst = 0;
    for (size_t i = 0; i < n_int; ++i) {
      if (start) start[i] = (uint32_t)len;
      while (at < n) {
        const uint8_t* ff = static_cast<const uint8_t*>(memchr(p + at, 0xFF, n - at));
        const size_t run = ff ? (size_t)(ff - (p + at)) : n - at;
        if (to && run) memcpy(to + len, p + at, run);
        len += run, at += run;
        if (!ff || at + 1 >= n || p[at + 1] != 0) break;
        if (to) to[len] = 0xFF;
        len += 1, at += 2;
      }
      if (i + 1 == n_int) break;
      if (at + 1 >= n) return false;                              // "restart marker RSTn missing"
      while (at < n && p[at] == 0xFF) ++at;
      if (at >= n || p[at] != 0xD0 + next_rst) return false;      // missing, or out of sequence
      ++at;
      next_rst = (next_rst + 1) & 7;
    }
    if (start) start[n_int] = (uint32_t)len;
    *total = len;
    return true;
  };
  size_t len = 0;
  if (n - pos > ((size_t)1 << 31)) fail(kUnsupported, "more than 2 GB of entropy-coded data (the interval plan's 32-bit sizes)");
  if (!walk(nullptr, nullptr, &len)) {                            // a marker is not where the walk needs it: the parser words the refusal
    size_t rec_needed = 0;
    (void)scan(nullptr, 0, &rec_needed);                          // throws what parse() reports
    fail(kInvalid, "restart markers are not where the intervals end");   // not reached: the walk applies scan()'s own marker rules
  }
  const size_t padded = (len + 3) / 4 * 4, total = stream_at + padded;
  if (needed) *needed = total;
  if (!dst || capacity < total) return kTooSmall;
  memset(dst + kPlanStreamOffset, 0, stream_at - kPlanStreamOffset);
  walk(dst + stream_at, reinterpret_cast<uint32_t*>(dst + kPlanStreamOffset), &len);
  memset(dst + stream_at + len, 0, padded - len);
  write_plan_head(dst, kIntervalPlanMagic, total, len, (uint32_t)n_int);
  return kOk;
}

// The geometry rules a plan header of either format must meet (what parse() would have produced); NULL: it does.
const char* plan_geometry_fault(const PlanHeader& ph) {
  const int w = (int)ph.width, h = (int)ph.height;
  if (w <= 0 || h <= 0 || w > kMaxDim || h > kMaxDim) return "frame size";
  if (ph.ncomp != 1 && ph.ncomp != 3) return "component count";
  const bool samp = ph.ncomp == 1 ? (ph.hs == 1 && ph.vs == 1) : ((ph.hs == 1 && ph.vs == 1) || (ph.hs == 2 && ph.vs == 1) || (ph.hs == 2 && ph.vs == 2));
  if (!samp) return "sampling factors";
  if (ph.mcus_x != ((uint32_t)w + 8 * ph.hs - 1) / (8 * ph.hs) || ph.mcus_y != ((uint32_t)h + 8 * ph.vs - 1) / (8 * ph.vs)) return "MCU grid";
  const uint32_t bpm = ph.ncomp == 1 ? 1 : ph.hs * ph.vs + 2;
  if (ph.n_blocks != ph.mcus_x * ph.mcus_y * bpm) return "block count";
  if (ph.bw[0] != ph.mcus_x * ph.hs || ph.bh[0] != ph.mcus_y * ph.vs) return "luma block grid";
  for (uint32_t c = 1; c < 3; ++c)
    if (ph.bw[c] != (c < ph.ncomp ? ph.mcus_x : 0u) || ph.bh[c] != (c < ph.ncomp ? ph.mcus_y : 0u)) return "chroma block grid";
  return nullptr;
}
}  // namespace

size_t plan_bound(int h, int w) {
  const size_t blocks = max_blocks(h, w);
  return blocks ? kPlanStreamOffset + ((blocks * kMaxBlockBits + 7) / 8 + 3) / 4 * 4 : 0;
}

int plan(const uint8_t* bytes, size_t n, long long frame, Info* info, void* out, size_t capacity, size_t* needed, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (needed) *needed = 0;
  Parser ps;
  ps.p = bytes, ps.n = n, ps.frame = frame, ps.msg = msg, ps.msg_cap = msg_cap;
  try {
    if (!bytes) ps.fail(kInvalid, "no data");
    if (out && (reinterpret_cast<uintptr_t>(out) & 3)) ps.fail(kInvalid, "the plan buffer is not 4-byte aligned");
    ps.segments(info);
    if (ps.restart) return kHostRoute;
    if (n - ps.pos > ((size_t)1 << 31)) return kHostRoute;       // the plan's 32-bit sizes
    return ps.write_plan(out, capacity, needed);
  } catch (const Failure& f) {
    return f.code;
  }
}

size_t max_blocks(int h, int w) {
  if (h <= 0 || w <= 0) return 0;
  const size_t b8x = ((size_t)w + 7) / 8, b8y = ((size_t)h + 7) / 8, b16x = ((size_t)w + 15) / 16, b16y = ((size_t)h + 15) / 16;
  size_t blocks = 3 * b8x * b8y;                                  // 4:4:4
  if (4 * b16x * b8y > blocks) blocks = 4 * b16x * b8y;          // 4:2:2
  if (6 * b16x * b16y > blocks) blocks = 6 * b16x * b16y;        // 4:2:0
  return blocks;
}

size_t record_bound(int h, int w) {
  const size_t blocks = max_blocks(h, w);
  return blocks ? record_bytes(blocks, 64 * blocks) : 0;
}

size_t planes_bytes(const RecordHeader& hd) {
  size_t t = 0;
  for (uint32_t c = 0; c < hd.ncomp && c < 3; ++c) t += 64 * (size_t)hd.bw[c] * hd.bh[c];
  return t;
}

int parse(const uint8_t* bytes, size_t n, long long frame, Info* info, void* record, size_t capacity, size_t* needed, char* msg,
          size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (needed) *needed = 0;
  Parser ps;
  ps.p = bytes, ps.n = n, ps.frame = frame, ps.msg = msg, ps.msg_cap = msg_cap;
  try {
    if (!bytes) ps.fail(kInvalid, "no data");
    if (record && (reinterpret_cast<uintptr_t>(record) & 3)) ps.fail(kInvalid, "the record buffer is not 4-byte aligned");
    ps.segments(info);
    return ps.scan(record, capacity, needed);
  } catch (const Failure& f) {
    return f.code;
  }
}

int probe(const uint8_t* bytes, size_t n, long long frame, Info* info, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  Parser ps;
  ps.p = bytes, ps.n = n, ps.frame = frame, ps.msg = msg, ps.msg_cap = msg_cap;
  try {
    if (!bytes) ps.fail(kInvalid, "no data");
    ps.segments(info);
    return kOk;
  } catch (const Failure& f) {
    return f.code;
  }
}

int check_plan(const void* plan, size_t bytes, char* msg, size_t msg_cap) {
  auto bad = [&](const char* what) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "JPEG plan: %s", what);
    return kInvalid;
  };
  if (!plan || bytes < kPlanStreamOffset || (reinterpret_cast<uintptr_t>(plan) & 3)) return bad("shorter than its header and tables, or misaligned");
  PlanHeader ph;
  memcpy(&ph, plan, sizeof ph);
  if (ph.magic != kPlanMagic) return bad("wrong magic");
  if (ph.bytes != bytes) return bad("its length field differs from the bytes handed in");
  if (ph.restart != 0) return bad("a restart interval");
  if (ph.stream_bytes > (1u << 31) || kPlanStreamOffset + ((size_t)ph.stream_bytes + 3) / 4 * 4 != bytes || ph.stream_bits != 8 * (uint64_t)ph.stream_bytes)
    return bad("its sizes do not add up to its length");
  if (const char* what = plan_geometry_fault(ph)) return bad(what);
  return kOk;
}

size_t plan_intervals_bound(int h, int w) {
  const size_t blocks = max_blocks(h, w);                         // at most one interval per MCU, so at most one per block
  return blocks ? interval_stream_offset(blocks) + ((blocks * kMaxBlockBits + 7) / 8 + blocks + 3) / 4 * 4 : 0;
}

int plan_intervals(const uint8_t* bytes, size_t n, long long frame, Info* info, void* out, size_t capacity, size_t* needed, char* msg, size_t msg_cap) {
  if (msg && msg_cap) msg[0] = 0;
  if (needed) *needed = 0;
  Parser ps;
  ps.p = bytes, ps.n = n, ps.frame = frame, ps.msg = msg, ps.msg_cap = msg_cap;
  try {
    if (!bytes) ps.fail(kInvalid, "no data");
    if (out && (reinterpret_cast<uintptr_t>(out) & 3)) ps.fail(kInvalid, "the plan buffer is not 4-byte aligned");
    ps.segments(info);
    if (!ps.restart) return kNoRestart;
    return ps.write_interval_plan(out, capacity, needed);
  } catch (const Failure& f) {
    return f.code;
  }
}

int check_plan_intervals(const void* plan, size_t bytes, char* msg, size_t msg_cap) {
  auto bad = [&](const char* what) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "JPEG interval plan: %s", what);
    return kInvalid;
  };
  if (!plan || bytes < interval_stream_offset(1) || (reinterpret_cast<uintptr_t>(plan) & 3)) return bad("shorter than its header and tables, or misaligned");
  PlanHeader ph;
  memcpy(&ph, plan, sizeof ph);
  if (ph.magic != kIntervalPlanMagic) return bad("wrong magic");
  if (ph.bytes != bytes) return bad("its length field differs from the bytes handed in");
  if (const char* what = plan_geometry_fault(ph)) return bad(what);
  if (ph.restart == 0 || ph.restart > 65535u) return bad("a restart interval outside 1..65535");
  const size_t n_int = interval_count((size_t)ph.mcus_x * ph.mcus_y, ph.restart), stream_at = interval_stream_offset(n_int);
  if (ph.reserved != n_int) return bad("its interval count is not ceil(MCUs / restart interval)");
  if (ph.stream_bytes > (1u << 31) || stream_at > bytes || stream_at + ((size_t)ph.stream_bytes + 3) / 4 * 4 != bytes || ph.stream_bits != 8 * (uint64_t)ph.stream_bytes)
    return bad("its sizes do not add up to its length");
  const uint32_t* start = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(plan) + kPlanStreamOffset);
  if (start[0] != 0) return bad("the first interval does not start at byte 0");
  for (size_t i = 0; i < n_int; ++i)
    if (start[i + 1] < start[i]) return bad("interval starts are not monotone");
  if (start[n_int] != ph.stream_bytes) return bad("the closing interval start differs from the stream length");
  return kOk;
}

int check_record(const void* record, size_t bytes, int h, int w, char* msg, size_t msg_cap) {
  auto bad = [&](const char* what) {
    if (msg && msg_cap) snprintf(msg, msg_cap, "JPEG record: %s", what);
    return kInvalid;
  };
  if (!record || bytes < kOffsetsOffset + 4 || (reinterpret_cast<uintptr_t>(record) & 3)) return bad("too short or misaligned");
  RecordHeader hd;
  memcpy(&hd, record, sizeof hd);
  if (hd.magic != kMagic) return bad("wrong magic");
  if (hd.bytes != bytes) return bad("its length field differs from the bytes handed in");
  if ((int)hd.width != w || (int)hd.height != h || w <= 0 || h <= 0 || w > kMaxDim || h > kMaxDim) return bad("its frame size differs from h x w");
  if (hd.ncomp != 1 && hd.ncomp != 3) return bad("component count");
  const bool samp = hd.ncomp == 1 ? (hd.hs == 1 && hd.vs == 1) : ((hd.hs == 1 && hd.vs == 1) || (hd.hs == 2 && hd.vs == 1) || (hd.hs == 2 && hd.vs == 2));
  if (!samp) return bad("sampling factors");
  if (hd.mcus_x != ((uint32_t)w + 8 * hd.hs - 1) / (8 * hd.hs) || hd.mcus_y != ((uint32_t)h + 8 * hd.vs - 1) / (8 * hd.vs)) return bad("MCU grid");
  const uint32_t bpm = hd.ncomp == 1 ? 1 : hd.hs * hd.vs + 2;
  if (hd.n_blocks != hd.mcus_x * hd.mcus_y * bpm) return bad("block count");
  if (hd.bw[0] != hd.mcus_x * hd.hs || hd.bh[0] != hd.mcus_y * hd.vs) return bad("luma block grid");
  for (uint32_t c = 1; c < hd.ncomp; ++c)
    if (hd.bw[c] != hd.mcus_x || hd.bh[c] != hd.mcus_y) return bad("chroma block grid");
  if (record_bytes(hd.n_blocks, hd.n_coef) != bytes) return bad("its sizes do not add up to its length");
  const uint32_t* off = reinterpret_cast<const uint32_t*>(static_cast<const uint8_t*>(record) + kOffsetsOffset);
  if (off[0] != 0) return bad("the first offset is not 0");
  for (uint32_t b = 0; b < hd.n_blocks; ++b)
    if (off[b + 1] < off[b] || off[b + 1] - off[b] > 64) return bad("block offsets are not monotone in steps of at most 64");
  if (off[hd.n_blocks] != hd.n_coef) return bad("the closing offset differs from the stream length");
  return kOk;
}

}  // namespace jpeg
}  // namespace gtx
