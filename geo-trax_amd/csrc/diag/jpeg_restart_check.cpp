// Stand-alone check of jpeg::plan_intervals() (csrc/jpeg_parse.cpp) and jpeg::emit_restart() (csrc/jpeg_emit.cpp) for the
// sanitizers (make -C geo-trax_amd jpegrestartcheck): no GPU, no Python; the counterpart of jpeg_plan_check.cpp. Every input sits
// in a heap block of exactly its size and every output in one of exactly the size asked for, so a read or write one byte out of
// bounds is an AddressSanitizer report. Every fixture's record is emitted at several restart intervals; each file must parse back
// to the record, its interval plan must pass check_plan_intervals() and hold one start per interval; a frame plan_intervals()
// refuses must be one parse() refuses with the same status and message. Then every truncation of one restart file and seeded
// single-byte corruptions of another.
//
//   jpeg_restart_check <fixture dir> [corruptions]
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../jpeg_emit.hpp"
#include "../jpeg_parse.hpp"

namespace jp = gtx::jpeg;

static std::vector<uint8_t> slurp(const std::string& path) {
  std::vector<uint8_t> v;
  FILE* f = fopen(path.c_str(), "rb");
  if (!f) return v;
  uint8_t buf[4096];
  size_t k;
  while ((k = fread(buf, 1, sizeof buf, f)) > 0) v.insert(v.end(), buf, buf + k);
  fclose(f);
  return v;
}

// 0: a consistent interval plan, 3: no restart interval, <0: refused as parse() refuses; anything else ends the check.
static int run_plan(const uint8_t* src, size_t n) {
  uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
  memcpy(data, src, n);
  jp::Info info, pinfo;
  size_t needed = 0, rec_needed = 0;
  char msg[256] = "", pmsg[256] = "";
  int rc = jp::plan_intervals(data, n, 0, &info, nullptr, 0, &needed, msg, sizeof msg);
  if (rc < 0) {
    const int prc = jp::parse(data, n, 0, &pinfo, nullptr, 0, &rec_needed, pmsg, sizeof pmsg);
    if (!msg[0] || rc != prc || strcmp(msg, pmsg) != 0) { fprintf(stderr, "refusal %d '%s' where parse() says %d '%s'\n", rc, msg, prc, pmsg); exit(2); }
    free(data);
    return rc;
  }
  if (rc == jp::kNoRestart) {
    if (needed != 0) { fprintf(stderr, "a frame without restart interval with a plan size\n"); exit(2); }
    free(data);
    return rc;
  }
  if (rc != jp::kTooSmall || needed < jp::interval_stream_offset(1) || needed % 4) { fprintf(stderr, "size query returned %d, needed %zu\n", rc, needed); exit(2); }
  uint8_t* out = static_cast<uint8_t*>(malloc(needed));
  memset(out, 0xAB, needed);
  size_t again = 0;
  rc = jp::plan_intervals(data, n, 0, &info, out, needed, &again, msg, sizeof msg);
  if (rc != 0 || again != needed) { fprintf(stderr, "second pass returned %d, %zu of %zu bytes: %s\n", rc, again, needed, msg); exit(2); }
  if (jp::check_plan_intervals(out, needed, msg, sizeof msg) != 0) { fprintf(stderr, "inconsistent interval plan: %s\n", msg); exit(2); }
  if (jp::check_plan(out, needed, msg, sizeof msg) == 0) { fprintf(stderr, "check_plan() accepts an interval plan\n"); exit(2); }
  if (needed > jp::plan_intervals_bound(info.height, info.width) && jp::parse(data, n, 0, &pinfo, nullptr, 0, &rec_needed, pmsg, sizeof pmsg) >= 0) {
    fprintf(stderr, "the interval plan of a decodable frame (%zu bytes) exceeds the bound\n", needed);
    exit(2);
  }
  if (needed > 4) {                                             // one word short: must report the size, not write past the end
    uint8_t* small = static_cast<uint8_t*>(malloc(needed - 4));
    if (jp::plan_intervals(data, n, 0, &info, small, needed - 4, &again, msg, sizeof msg) != jp::kTooSmall || again != needed) { fprintf(stderr, "short plan not reported\n"); exit(2); }
    free(small);
  }
  free(out);
  free(data);
  return 0;
}

// The record of one fixture emitted with `restart`: the file (exactly sized), checked against the parser.
static std::vector<uint8_t> emit_checked(const uint8_t* rec, size_t rec_bytes, unsigned restart) {
  char msg[256] = "";
  size_t n = 0, again = 0;
  int rc = jp::emit_restart(rec, rec_bytes, restart, nullptr, 0, &n, msg, sizeof msg);
  if (rc != jp::kTooSmall || n == 0) { fprintf(stderr, "emit_restart size query returned %d: %s\n", rc, msg); exit(2); }
  uint8_t* out = static_cast<uint8_t*>(malloc(n));
  rc = jp::emit_restart(rec, rec_bytes, restart, out, n, &again, msg, sizeof msg);
  if (rc != 0 || again != n) { fprintf(stderr, "emit_restart returned %d, %zu of %zu bytes: %s\n", rc, again, n, msg); exit(2); }
  if (n > 1) {
    uint8_t* small = static_cast<uint8_t*>(malloc(n - 1));
    if (jp::emit_restart(rec, rec_bytes, restart, small, n - 1, &again, msg, sizeof msg) != jp::kTooSmall || again != n) { fprintf(stderr, "short output not reported\n"); exit(2); }
    free(small);
  }
  jp::Info info;
  size_t needed = 0;
  jp::parse(out, n, 0, &info, nullptr, 0, &needed, msg, sizeof msg);
  if (needed != rec_bytes) { fprintf(stderr, "restart %u: the file parses to %zu bytes, the record has %zu: %s\n", restart, needed, rec_bytes, msg); exit(2); }
  uint32_t* back = static_cast<uint32_t*>(malloc(needed));
  if (jp::parse(out, n, 0, &info, back, needed, &again, msg, sizeof msg) != 0 || memcmp(back, rec, rec_bytes) != 0) { fprintf(stderr, "restart %u: the file does not parse back to the record\n", restart); exit(2); }
  free(back);
  std::vector<uint8_t> v(out, out + n);
  free(out);
  return v;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <fixture dir> [corruptions]\n", argv[0]); return 64; }
  const std::string dir = argv[1];
  const int n_corrupt = argc > 2 ? atoi(argv[2]) : 2000;
  int n_files = 0, n_emitted = 0;
  std::vector<uint8_t> keep_row, keep_one;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 5 || name.substr(name.size() - 4) != ".jpg") continue;
      const std::vector<uint8_t> v = slurp(dir + "/" + name);
      const int rc = run_plan(v.data(), v.size());
      const int want = name.find("progressive") != std::string::npos ? jp::kUnsupported : name.find("_rst") != std::string::npos ? 0 : jp::kNoRestart;
      if (rc != want) { fprintf(stderr, "%s: status %d, expected %d\n", name.c_str(), rc, want); return 1; }
      ++n_files;
      if (rc < 0) continue;
      jp::Info info;
      size_t needed = 0;
      char msg[256];
      jp::parse(v.data(), v.size(), 0, &info, nullptr, 0, &needed, msg, sizeof msg);
      uint32_t* rec = static_cast<uint32_t*>(malloc(needed));
      size_t again = 0;
      if (jp::parse(v.data(), v.size(), 0, &info, rec, needed, &again, msg, sizeof msg) != 0) { fprintf(stderr, "%s: %s\n", name.c_str(), msg); return 1; }
      jp::RecordHeader hd;
      memcpy(&hd, rec, sizeof hd);
      const unsigned n_mcus = hd.mcus_x * hd.mcus_y;
      if (name.find("q100") == std::string::npos && name.find("opt") == std::string::npos) {   // (coefficients the Annex K.3 tables may not code)
        const unsigned rs[] = {0, 1, 3, 4, hd.mcus_x, n_mcus, n_mcus + 5, 65535};
        for (unsigned r : rs) {
          const std::vector<uint8_t> file = emit_checked(reinterpret_cast<const uint8_t*>(rec), needed, r);
          const int prc = run_plan(file.data(), file.size());
          if (prc != (r ? 0 : jp::kNoRestart)) { fprintf(stderr, "%s at restart %u: plan_intervals() returned %d\n", name.c_str(), r, prc); return 1; }
          ++n_emitted;
          if (name == "p70x45_420.jpg" && r == 1) keep_one = file;
          if (name == "p70x45_420.jpg" && r == hd.mcus_x) keep_row = file;
        }
        char emsg[256];
        size_t en = 0;
        if (jp::emit_restart(rec, needed, 65536, nullptr, 0, &en, emsg, sizeof emsg) != jp::kInvalid) { fprintf(stderr, "a restart interval of 65536 was accepted\n"); return 1; }
      }
      free(rec);
    }
    closedir(d);
  }
  if (n_files < 10 || keep_one.empty() || keep_row.empty()) { fprintf(stderr, "only %d fixtures in %s\n", n_files, dir.c_str()); return 1; }

  int cut_ok = 0;
  for (size_t len = 0; len < keep_row.size(); ++len) cut_ok += run_plan(keep_row.data(), len) == 0;
  if (cut_ok == 0) { fprintf(stderr, "no truncation gave an interval plan\n"); return 1; }

  uint64_t s = 0x9E3779B97F4A7C15ull;
  int survived = 0;
  for (int k = 0; k < n_corrupt; ++k) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const size_t at = (size_t)((s >> 33) % keep_one.size());
    const uint8_t was = keep_one[at];
    keep_one[at] = (uint8_t)(was ^ (1 + ((s >> 12) % 255)));
    survived += run_plan(keep_one.data(), keep_one.size()) == 0;
    keep_one[at] = was;
  }
  printf("jpeg_restart_check: %d fixtures, %d files emitted with restart intervals and planned, %zu truncations (%d plans), %d corruptions (%d plans)\n", n_files,
         n_emitted, keep_row.size(), cut_ok, n_corrupt, survived);
  return 0;
}
