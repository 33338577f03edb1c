// Stand-alone check of csrc/jpeg_emit.cpp for the sanitizers (make -C geo-trax_amd jpegemitcheck): no GPU, no Python. Every
// record sits in a heap block of exactly its size and every output in one of exactly the size the emitter asked for, so a read or
// write one byte out of bounds is an AddressSanitizer report. Inputs: the record of every fixture the parser accepts (emitted,
// parsed again: the same record byte for byte), and seeded single-byte corruptions of one fixture's record (refused with a
// message, or emitted into a file the parser reads).
//
//   jpeg_emit_check <fixture dir> [corruption fixture] [corruptions]
#include <dirent.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../jpeg_emit.hpp"

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

// the file's record in a heap block of exactly its size (NULL: the parser refuses the file)
static uint8_t* record_of(const uint8_t* data, size_t n, size_t* bytes) {
  jp::Info info;
  char msg[256] = "";
  if (jp::parse(data, n, 0, &info, nullptr, 0, bytes, msg, sizeof msg) != jp::kTooSmall) return nullptr;
  uint8_t* rec = static_cast<uint8_t*>(malloc(*bytes));
  if (jp::parse(data, n, 0, &info, rec, *bytes, bytes, msg, sizeof msg) != 0) { fprintf(stderr, "second parse failed: %s\n", msg); exit(2); }
  return rec;
}

// 0: emitted (the file in *file), <0: refused with a message; anything else is a failure of the check (exit).
static int run(const uint8_t* rec, size_t bytes, std::vector<uint8_t>* file) {
  char msg[256] = "";
  size_t n = 0, again = 0;
  int rc = jp::emit(rec, bytes, nullptr, 0, &n, msg, sizeof msg);
  if (rc < 0) {
    if (!msg[0]) { fprintf(stderr, "a refusal without a message (status %d)\n", rc); exit(2); }
    return rc;
  }
  if (rc != jp::kTooSmall || n < 100) { fprintf(stderr, "size query returned %d, %zu bytes\n", rc, n); exit(2); }
  uint8_t* out = static_cast<uint8_t*>(malloc(n));
  rc = jp::emit(rec, bytes, out, n, &again, msg, sizeof msg);
  if (rc != 0 || again != n) { fprintf(stderr, "second pass returned %d, %zu of %zu bytes: %s\n", rc, again, n, msg); exit(2); }
  uint8_t* small = static_cast<uint8_t*>(malloc(n - 1));           // one byte short: the size, nothing past the end
  if (jp::emit(rec, bytes, small, n - 1, &again, msg, sizeof msg) != jp::kTooSmall || again != n) { fprintf(stderr, "short buffer not reported\n"); exit(2); }
  if (memcmp(small, out, n - 1) != 0) { fprintf(stderr, "the short buffer's bytes differ\n"); exit(2); }
  free(small);
  if (file) file->assign(out, out + n);
  free(out);
  return 0;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: %s <fixture dir> [corruption fixture] [corruptions]\n", argv[0]); return 64; }
  const std::string dir = argv[1], corrupt_name = argc > 2 ? argv[2] : "p70x45_420.jpg";
  const int n_corrupt = argc > 3 ? atoi(argv[3]) : 4000;
  int n_files = 0;
  if (DIR* d = opendir(dir.c_str())) {
    while (dirent* e = readdir(d)) {
      const std::string name = e->d_name;
      if (name.size() < 5 || name.substr(name.size() - 4) != ".jpg") continue;
      const std::vector<uint8_t> v = slurp(dir + "/" + name);
      size_t bytes = 0, bytes2 = 0;
      uint8_t* rec = record_of(v.data(), v.size(), &bytes);
      if (!rec) continue;                                          // a variant the parser refuses
      std::vector<uint8_t> file;
      if (run(rec, bytes, &file) != 0) { fprintf(stderr, "%s: its record was refused\n", name.c_str()); return 1; }
      uint8_t* data = static_cast<uint8_t*>(malloc(file.size()));
      memcpy(data, file.data(), file.size());
      uint8_t* rec2 = record_of(data, file.size(), &bytes2);
      if (!rec2 || bytes2 != bytes || memcmp(rec, rec2, bytes) != 0) { fprintf(stderr, "%s: the emitted file parses to another record\n", name.c_str()); return 1; }
      free(rec2), free(data), free(rec);
      ++n_files;
    }
    closedir(d);
  }
  if (n_files < 10) { fprintf(stderr, "only %d fixtures in %s\n", n_files, dir.c_str()); return 1; }

  const std::vector<uint8_t> cv = slurp(dir + "/" + corrupt_name);
  size_t bytes = 0;
  uint8_t* rec = cv.empty() ? nullptr : record_of(cv.data(), cv.size(), &bytes);
  if (!rec) { fprintf(stderr, "%s is missing or refused\n", corrupt_name.c_str()); return 1; }
  uint64_t s = 0x9E3779B97F4A7C15ull;
  int emitted = 0;
  for (int k = 0; k < n_corrupt; ++k) {
    s = s * 6364136223846793005ull + 1442695040888963407ull;
    // one corruption in three hits the header, the tables or the first offsets, where the sizes are
    const size_t span = (k % 3 == 0) ? (jp::kOffsetsOffset + 64 < bytes ? jp::kOffsetsOffset + 64 : bytes) : bytes;
    const size_t at = (size_t)((s >> 33) % span);
    const uint8_t was = rec[at];
    rec[at] = (uint8_t)(was ^ (1 + ((s >> 12) % 255)));
    std::vector<uint8_t> file;
    if (run(rec, bytes, &file) == 0) {
      ++emitted;
      uint8_t* data = static_cast<uint8_t*>(malloc(file.size()));
      memcpy(data, file.data(), file.size());
      size_t b2 = 0;
      uint8_t* rec2 = record_of(data, file.size(), &b2);
      if (!rec2) { fprintf(stderr, "corruption %d at byte %zu: the emitted file is refused by the parser\n", k, at); return 1; }
      free(rec2), free(data);
    }
    rec[at] = was;
  }
  for (size_t len = 0; len < bytes; len += (len < 600 ? 1 : 97)) {  // truncated records: refused, never read past their end
    uint8_t* cut = static_cast<uint8_t*>(malloc(len ? len : 1));
    memcpy(cut, rec, len);
    if (run(cut, len, nullptr) == 0) { fprintf(stderr, "a record cut to %zu of %zu bytes was emitted\n", len, bytes); return 1; }
    free(cut);
  }
  free(rec);
  printf("jpeg_emit_check: %d fixtures round-tripped, %d corruptions (%d emitted and parsed again)\n", n_files, n_corrupt, emitted);
  return 0;
}
