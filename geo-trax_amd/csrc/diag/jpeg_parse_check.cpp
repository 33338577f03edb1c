// Stand-alone check of csrc/jpeg_parse.cpp for the sanitizers (make -C geo-trax_amd jpegcheck): no GPU, no Python. Every input
// sits in a heap block of exactly its size and every record in one of exactly the size the parser asked for, so a read or write
// one byte out of bounds is an AddressSanitizer report. Inputs: every .jpg of the fixture folder; every truncation of one
// fixture; seeded single-byte corruptions of a fixture with restart markers.
//
//   jpeg_parse_check <fixture dir> [truncation fixture] [corruption fixture] [corruptions]
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

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

// 0: decoded into a consistent record, <0: refused with a message; anything else is a failure of the check (exit).
static int run(const uint8_t* src, size_t n, jp::Info* info_out) {
  uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
  memcpy(data, src, n);
  jp::Info info;
  size_t needed = 0;
  char msg[256] = "";
  int rc = jp::parse(data, n, 0, &info, nullptr, 0, &needed, msg, sizeof msg);
  if (rc < 0) {
    if (!msg[0]) { fprintf(stderr, "a refusal without a message (status %d)\n", rc); exit(2); }
    free(data);
    return rc;
  }
  if (rc != jp::kTooSmall || needed == 0) { fprintf(stderr, "size query returned %d, needed %zu\n", rc, needed); exit(2); }
  uint8_t* rec = static_cast<uint8_t*>(malloc(needed));
  size_t again = 0;
  rc = jp::parse(data, n, 0, &info, rec, needed, &again, msg, sizeof msg);
  if (rc != 0 || again != needed) { fprintf(stderr, "second pass returned %d, %zu of %zu bytes: %s\n", rc, again, needed, msg); exit(2); }
  if (jp::check_record(rec, needed, info.height, info.width, msg, sizeof msg) != 0) { fprintf(stderr, "inconsistent record: %s\n", msg); exit(2); }
  if (needed > jp::record_bound(info.height, info.width)) { fprintf(stderr, "record of %zu bytes exceeds the bound\n", needed); exit(2); }
  if (needed > 4) {                                             // one byte short: must report the size, not write past the end
    uint8_t* small = static_cast<uint8_t*>(malloc(needed - 4));
    if (jp::parse(data, n, 0, &info, small, needed - 4, &again, msg, sizeof msg) != jp::kTooSmall || again != needed) { fprintf(stderr, "short record not reported\n"); exit(2); }
    free(small);
  }
  if (info_out) *info_out = info;
  free(rec);
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <fixture dir> [truncation fixture] [corruption fixture] [corruptions]\n", argv[0]); return 64; }
  const std::string dir = argv[1];
  const std::string trunc_name = argc > 2 ? argv[2] : "r17x9_420.jpg", corrupt_name = argc > 3 ? argv[3] : "p70x45_420_rst3.jpg";
  const int n_corrupt = argc > 4 ? atoi(argv[4]) : 2000;
  int n_files = 0, n_ok = 0;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 5 || name.substr(name.size() - 4) != ".jpg") continue;
      const std::vector<uint8_t> v = slurp(dir + "/" + name);
      const int rc = run(v.data(), v.size(), nullptr);
      const bool refused = name.find("progressive") != std::string::npos;
      if ((rc == 0) == refused) { fprintf(stderr, "%s: status %d\n", name.c_str(), rc); return 1; }
      ++n_files, n_ok += rc == 0;
    }
    closedir(d);
  }
  if (n_files < 10) { fprintf(stderr, "only %d fixtures in %s\n", n_files, dir.c_str()); return 1; }

  const std::vector<uint8_t> t = slurp(dir + "/" + trunc_name);
  int cut_ok = 0;
  for (size_t len = 0; len < t.size(); ++len) {
    const int rc = run(t.data(), len, nullptr);
    const bool in_eoi = len + 2 >= t.size();                     // only the trailing EOI is cut: the picture is complete
    if ((rc == 0) != in_eoi) { fprintf(stderr, "%s cut to %zu of %zu bytes: status %d\n", trunc_name.c_str(), len, t.size(), rc); return 1; }
    cut_ok += rc == 0;
  }

  std::vector<uint8_t> c = slurp(dir + "/" + corrupt_name);
  if (c.empty()) { fprintf(stderr, "%s is missing\n", corrupt_name.c_str()); return 1; }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  int survived = 0;
  for (int k = 0; k < n_corrupt; ++k) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const size_t at = (size_t)((s >> 33) % c.size());
    const uint8_t was = c[at];
    c[at] = (uint8_t)(was ^ (1 + ((s >> 12) % 255)));
    survived += run(c.data(), c.size(), nullptr) == 0;
    c[at] = was;
  }
  printf("jpeg_parse_check: %d fixtures (%d decoded), %zu truncations (%d decoded), %d corruptions (%d decoded)\n", n_files, n_ok, t.size(), cut_ok,
         n_corrupt, survived);
  return 0;
}
