// Stand-alone check of jpeg::plan() (csrc/jpeg_parse.cpp) for the sanitizers (make -C geo-trax_amd jpegplancheck): no GPU, no
// Python; the counterpart of jpeg_parse_check.cpp. Every input sits in a heap block of exactly its size and every plan in one of
// exactly the size plan() asked for, so a read or write one byte out of bounds is an AddressSanitizer report. A plan that is
// written must pass check_plan(), agree with probe() on the header, and hold the entropy-coded bytes the parser's bit reader
// would have fetched. Inputs: every .jpg of the fixture folder; every truncation of one fixture; seeded single-byte corruptions.
//
//   jpeg_plan_check <fixture dir> [truncation fixture] [corruption fixture] [corruptions]
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

// 0: a consistent plan, 2: handed to the host route, <0: refused with probe()'s status and message; anything else ends the check.
static int run(const uint8_t* src, size_t n) {
  uint8_t* data = static_cast<uint8_t*>(malloc(n ? n : 1));
  memcpy(data, src, n);
  jp::Info info, pinfo;
  size_t needed = 0;
  char msg[256] = "", pmsg[256] = "";
  int rc = jp::plan(data, n, 0, &info, nullptr, 0, &needed, msg, sizeof msg);
  const int prc = jp::probe(data, n, 0, &pinfo, pmsg, sizeof pmsg);
  if (rc < 0) {
    if (!msg[0] || rc != prc || strcmp(msg, pmsg) != 0) { fprintf(stderr, "refusal %d '%s' where probe() says %d '%s'\n", rc, msg, prc, pmsg); exit(2); }
    free(data);
    return rc;
  }
  if (prc != 0) { fprintf(stderr, "plan() accepts (%d) what probe() refuses: %s\n", rc, pmsg); exit(2); }
  if (rc == jp::kHostRoute) {
    if (needed != 0) { fprintf(stderr, "a host-route frame with a plan size\n"); exit(2); }
    free(data);
    return rc;
  }
  if (rc != jp::kTooSmall || needed < jp::kPlanStreamOffset || needed % 4) { fprintf(stderr, "size query returned %d, needed %zu\n", rc, needed); exit(2); }
  uint8_t* out = static_cast<uint8_t*>(malloc(needed));
  memset(out, 0xAB, needed);
  size_t again = 0;
  rc = jp::plan(data, n, 0, &info, out, needed, &again, msg, sizeof msg);
  if (rc != 0 || again != needed) { fprintf(stderr, "second pass returned %d, %zu of %zu bytes: %s\n", rc, again, needed, msg); exit(2); }
  if (jp::check_plan(out, needed, msg, sizeof msg) != 0) { fprintf(stderr, "inconsistent plan: %s\n", msg); exit(2); }
  jp::PlanHeader ph;
  memcpy(&ph, out, sizeof ph);
  if ((int)ph.width != pinfo.width || (int)ph.height != pinfo.height || (int)ph.ncomp != pinfo.ncomp || (int)ph.hs != pinfo.hs || (int)ph.vs != pinfo.vs) {
    fprintf(stderr, "the plan's header differs from probe()'s\n");
    exit(2);
  }
  if (needed > jp::plan_bound(info.height, info.width) && jp::parse(data, n, 0, &info, nullptr, 0, &again, msg, sizeof msg) >= 0) {
    fprintf(stderr, "the plan of a decodable frame (%zu bytes) exceeds the bound\n", needed);
    exit(2);
  }
  // the clean stream, stuffed again, is a prefix of the input's tail that ends where an FF is not followed by 00, or at the end
  std::vector<uint8_t> stuffed;
  for (uint32_t i = 0; i < ph.stream_bytes; ++i) {
    stuffed.push_back(out[jp::kPlanStreamOffset + i]);
    if (stuffed.back() == 0xFF) stuffed.push_back(0);
  }
  bool found = false;
  for (size_t at = 2; at + stuffed.size() <= n && !found; ++at) {
    if (!stuffed.empty() && memcmp(data + at, stuffed.data(), stuffed.size()) != 0) continue;
    const size_t end = at + stuffed.size();
    found = end == n || (data[end] == 0xFF && (end + 1 == n || data[end + 1] != 0));
  }
  if (!found) { fprintf(stderr, "the clean stream (%u bytes) is not the input's entropy-coded segment\n", ph.stream_bytes); exit(2); }
  for (size_t i = jp::kPlanStreamOffset + ph.stream_bytes; i < needed; ++i)
    if (out[i] != 0) { fprintf(stderr, "the padding behind the stream is not zero\n"); exit(2); }
  if (needed > 4) {                                             // one word short: must report the size, not write past the end
    uint8_t* small = static_cast<uint8_t*>(malloc(needed - 4));
    if (jp::plan(data, n, 0, &info, small, needed - 4, &again, msg, sizeof msg) != jp::kTooSmall || again != needed) { fprintf(stderr, "short plan not reported\n"); exit(2); }
    free(small);
  }
  free(out);
  free(data);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <fixture dir> [truncation fixture] [corruption fixture] [corruptions]\n", argv[0]); return 64; }
  const std::string dir = argv[1];
  const std::string trunc_name = argc > 2 ? argv[2] : "r17x9_420.jpg", corrupt_name = argc > 3 ? argv[3] : "p70x45_420.jpg";
  const int n_corrupt = argc > 4 ? atoi(argv[4]) : 2000;
  int n_files = 0, n_plans = 0, n_host = 0;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 5 || name.substr(name.size() - 4) != ".jpg") continue;
      const std::vector<uint8_t> v = slurp(dir + "/" + name);
      const int rc = run(v.data(), v.size());
      const int want = name.find("progressive") != std::string::npos ? jp::kUnsupported : name.find("_rst") != std::string::npos ? jp::kHostRoute : 0;
      if (rc != want) { fprintf(stderr, "%s: status %d, expected %d\n", name.c_str(), rc, want); return 1; }
      ++n_files, n_plans += rc == 0, n_host += rc == jp::kHostRoute;
    }
    closedir(d);
  }
  if (n_files < 10) { fprintf(stderr, "only %d fixtures in %s\n", n_files, dir.c_str()); return 1; }

  const std::vector<uint8_t> t = slurp(dir + "/" + trunc_name);
  int cut_ok = 0;
  for (size_t len = 0; len < t.size(); ++len) cut_ok += run(t.data(), len) == 0;
  if (cut_ok == 0) { fprintf(stderr, "no truncation of %s gave a plan\n", trunc_name.c_str()); return 1; }

  std::vector<uint8_t> c = slurp(dir + "/" + corrupt_name);
  if (c.empty()) { fprintf(stderr, "%s is missing\n", corrupt_name.c_str()); return 1; }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  int survived = 0;
  for (int k = 0; k < n_corrupt; ++k) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    const size_t at = (size_t)((s >> 33) % c.size());
    const uint8_t was = c[at];
    c[at] = (uint8_t)(was ^ (1 + ((s >> 12) % 255)));
    survived += run(c.data(), c.size()) == 0;
    c[at] = was;
  }
  printf("jpeg_plan_check: %d fixtures (%d plans, %d for the host route), %zu truncations (%d plans), %d corruptions (%d plans)\n", n_files, n_plans, n_host,
         t.size(), cut_ok, n_corrupt, survived);
  return 0;
}
