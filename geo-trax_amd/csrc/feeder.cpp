// Frame feeder: the read-ahead half of the reference's `cap.read()` (geotrax/extract.py:146) for sources whose
// frames sit uncompressed in a file (.y4m, .npy) or are produced by a host thread (image folders, a decoder).
//
// The reference reads one frame synchronously at the top of every loop iteration. At 4K that is 12.4 MB (I420)
// or 24.9 MB (BGR) per frame; done on the thread that also drives the detector it is the whole pipeline's pace.
// Here the read, the PCIe transfer and the colour conversion run beside the pipeline:
//
//   reader threads   pread() whole frames straight into a ring of pinned (hipHostMalloc) slots -- one copy out
//                    of the page cache, no intermediate bytes object, frames of a batch read in parallel;
//   uploader thread  hipMemcpyAsync of every slot to its place in a ring of device batches on the feeder's own
//                    stream (pinned memory: the copy engines do it), I420 slots through yuv420_to_bgr_kernel on the
//                    same stream, one event per batch;
//   consumer         gtx_feeder_next() hands out batches in clip order as device pointers; gtx_feeder_wait() makes the
//                    consumer's stream wait for the batch's event (no host thread blocks on the transfer);
//                    gtx_feeder_release() returns slots once the consumer's pass over them is complete.
//
// Push mode (no file): the caller's own thread hands host frames to gtx_feeder_push(), which copies them into the
// pinned ring; everything behind that is the same.
#include <fcntl.h>
#include <unistd.h>

#include <atomic>
#include <cerrno>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>

#include "../../include/gtx.h"
#include "api_guard.hpp"
#include "common.hpp"
#include "detector.hpp"
#include "geometry.hpp"
#include "jpeg.hpp"
#include "jpeg_entropy.hpp"
#include "jpeg_restart.hpp"

struct gtx_feeder {
  gtx_ctx ctx;                       // device + the copy stream
  bool own_stream = true;            // false: the stream belongs to the context the feeder was created on
  int h = 0, w = 0, kind = 0;        // kind 0: BGR u8 frames, 1: I420 planes, 2: compressed JPEG frames (the slot holds the decoded record)
  int B = 1, ring = 4;
  size_t src_bytes = 0, bgr_bytes = 0;
  uint8_t* pinned = nullptr;         // [ring][B][src_bytes], hipHostMalloc
  gtx::DevBuf dev, dev_yuv;          // [ring][B][bgr_bytes]; [ring][B][src_bytes] (I420 only)
  gtx::DevBuf dev_rec, dev_planes;   // JPEG only: one record and its sample planes (the copy stream runs the frames in order)
  std::vector<hipEvent_t> ev;        // per ring slot: the batch's uploads (and conversions) are complete

  int fd = -1;
  std::vector<std::string> paths;    // JPEG file mode: the files frames are read from ...
  int one_fd = -1;                   // ... one file (a clip): opened once; several (a file per frame): each reader thread opens the
                                     //     file of the frame it took, reads it and closes it again, so a folder of any length
                                     //     costs one descriptor per thread, never one per frame
  std::vector<int32_t> file_index;   // ... which of them holds frame i ...
  std::vector<int64_t> lengths;      // ... and how many compressed bytes it has there (at offsets[i])
  std::vector<uint32_t> slot_len;    // [ring*B] JPEG only: bytes of the record in the pinned slot
  // JPEG, the GPU entropy route (gtx_feeder_set_jpeg_entropy): a reader thread writes the frame's plan (jpeg::plan(): header walk and
  // unstuffing) into the slot instead of its record and keeps the compressed bytes; the uploader runs the entropy chain in front of
  // the pixel kernels and copies the frame's status word back; next() sends a frame whose status is not 0 to the host parser.
  std::unique_ptr<gtx::JpegEntropy> entropy;
  gtx::DevBuf dev_plan, fb_rec, fb_planes;   // the plan in HBM; record and planes of a frame next() decodes again on the host
  std::vector<uint8_t> slot_tag;     // [ring*B] what the pinned slot holds: 0 a record, 1 a plan, 2 an interval plan, 3 a record the restart route handed back
  std::vector<std::vector<uint8_t>> slot_src;   // [ring*B] the compressed bytes of the slot's frame
  uint32_t* h_status = nullptr;      // pinned [ring*B][2]: the entropy chain's status and rounds used
  std::atomic<int64_t> stats[3] = {{0}, {0}, {0}};   // frames decoded by the GPU / by the host because plan() said so / by the host after a GPU status
  // JPEG, the restart-interval route (gtx_feeder_set_jpeg_restart): a frame that has a restart interval gets an interval plan
  // (jpeg::plan_intervals()) in its slot, whichever way the other frames go. The uploader copies the plans of a batch side by
  // side into HBM and, when the batch is complete, decodes all their intervals in one launch (csrc/jpeg_restart.hip).
  std::unique_ptr<gtx::JpegRestart> restart;
  gtx::DevBuf rs_plan, rs_rec;       // [B][src_bytes] each: the batch's interval plans and their records
  uint32_t* h_rstatus = nullptr;     // pinned [ring*B]: the restart chain's status
  std::atomic<int64_t> rstats[3] = {{0}, {0}, {0}};   // frames decoded by the interval route / handed back to the reader thread / decoded again after a GPU status
  int64_t dead_from = -1;            // next(): the batch a frame of which the host parser refused too; nothing from it on is delivered
  std::map<int64_t, std::string> bad;   // JPEG only: frames that could not be decoded; the uploader reports one when it reaches it
  std::vector<int64_t> offsets;      // file mode: payload offset of every frame to deliver, in delivery order
  std::vector<const uint8_t*> mem;   // memory mode: the frames as host pointers (the caller keeps them alive), in delivery order
  std::vector<std::thread> readers;
  std::thread uploader;

  std::mutex m;
  std::condition_variable cv;
  int64_t n_frames = -1;             // -1: not known yet (push mode before gtx_feeder_finish)
  int64_t next_read = 0;             // next frame a reader thread takes (file mode) / next frame pushed
  std::vector<int64_t> slot_frame;   // [ring*B]: frame whose bytes the pinned slot holds, -1 = none
  int64_t issued = 0;                // batches whose copies are on the stream (event recorded)
  int64_t handed = 0;                // batches returned by next()
  int64_t released = 0;              // batches whose slots may be overwritten
  bool stop = false;
  std::string error;                 // first failure of a worker thread

  int64_t n_batches() const { return n_frames < 0 ? -1 : (n_frames + B - 1) / B; }
  size_t slot_of(int64_t frame) const { return (size_t)((frame / B) % ring) * B + (size_t)(frame % B); }

  ~gtx_feeder() {
    {
      std::lock_guard<std::mutex> lk(m);
      stop = true;
    }
    cv.notify_all();
    for (auto& t : readers) if (t.joinable()) t.join();
    if (uploader.joinable()) uploader.join();
    (void)hipSetDevice(ctx.device);
    if (ctx.stream) (void)hipStreamSynchronize(ctx.stream);
    for (auto e : ev) (void)hipEventDestroy(e);
    if (pinned) (void)hipHostFree(pinned);
    if (h_status) (void)hipHostFree(h_status);
    if (h_rstatus) (void)hipHostFree(h_rstatus);
    if (fd >= 0) ::close(fd);
    if (one_fd >= 0) ::close(one_fd);
    if (!own_stream) ctx.stream = nullptr;   // ~gtx_ctx must not destroy a borrowed stream
  }

  void set_error(const std::string& what) {
    std::lock_guard<std::mutex> lk(m);
    if (error.empty()) error = what;
    stop = true;
    cv.notify_all();
  }

  // JPEG: entropy-decodes one compressed frame into frame i's pinned slot and checks the record the kernels will index by.
  // false: `why` says what is wrong with the frame (nothing of it is delivered).
  bool decode_into_slot(int64_t i, const uint8_t* data, size_t len, std::string& why) {
    const size_t s = slot_of(i);
    uint8_t* dst = pinned + s * src_bytes;
    gtx::jpeg::Info info;
    size_t needed = 0;
    char msg[512];
    const int rc = gtx::jpeg::parse(data, len, (long long)i, &info, dst, src_bytes, &needed, msg, sizeof msg);
    if (rc < 0) {
      why = msg;
      return false;
    }
    if (info.height != h || info.width != w) {
      why = "JPEG frame " + std::to_string(i) + ": its size " + std::to_string(info.width) + " x " + std::to_string(info.height) + " differs from the feeder's " +
            std::to_string(w) + " x " + std::to_string(h);
      return false;
    }
    if (rc != 0 || gtx::jpeg::check_record(dst, needed, h, w, msg, sizeof msg) != 0) {
      why = rc != 0 ? "JPEG frame " + std::to_string(i) + ": the record does not fit the slot" : std::string(msg);
      return false;
    }
    slot_len[s] = (uint32_t)needed;
    return true;
  }

  // JPEG: frame i's compressed bytes -> its pinned slot, as a plan on the GPU entropy route and as the record otherwise. A frame
  // plan() hands back (a restart interval), one whose plan does not fit the slot and one whose size is not the feeder's (the host
  // route words that refusal) are decoded here as on the host route.
  bool fill_slot(int64_t i, const uint8_t* data, size_t len, std::string& why) {
    const size_t s = slot_of(i);
    if (!entropy && !restart) return decode_into_slot(i, data, len, why);
    slot_tag[s] = 0;
    gtx::jpeg::Info info;
    size_t needed = 0;
    char msg[512];
    if (restart) {
      // Only bad or odd frames pay twice here, and harmlessly: where a marker is out of place plan_intervals() has already run the
      // parser's scan to word its refusal and decode_into_slot() below runs parse() once more, so that the message is the host
      // route's whatever the cause; a frame of another size had its plan written into the slot before parse() writes over it.
      const int rc = gtx::jpeg::plan_intervals(data, len, (long long)i, &info, pinned + s * src_bytes, src_bytes, &needed, msg, sizeof msg);
      if (rc == gtx::jpeg::kOk && info.height == h && info.width == w) {
        if (slot_src[s].data() != data) slot_src[s].assign(data, data + len);
        slot_len[s] = (uint32_t)needed;
        slot_tag[s] = 2;
        return true;
      }
      if (rc != gtx::jpeg::kNoRestart) {                       // refused, too large for the slot or of another size: the host route decodes it or words the refusal
        const bool ok = decode_into_slot(i, data, len, why);
        if (ok) slot_tag[s] = 3;
        return ok;
      }
      if (!entropy) return decode_into_slot(i, data, len, why);
    }
    const int rc = gtx::jpeg::plan(data, len, (long long)i, &info, pinned + s * src_bytes, src_bytes, &needed, msg, sizeof msg);
    if (rc < 0) {
      why = msg;
      return false;
    }
    if (rc != gtx::jpeg::kOk || info.height != h || info.width != w) {
      return decode_into_slot(i, data, len, why);             // (counted when the frame is delivered: settle_batch)
    }
    if (slot_src[s].data() != data) slot_src[s].assign(data, data + len);
    slot_len[s] = (uint32_t)needed;
    slot_tag[s] = 1;
    return true;
  }

  // Frame i is in its slot (why empty) or can never be (the uploader reports it after the batches before it).
  void publish(int64_t i, const std::string& why) {
    {
      std::lock_guard<std::mutex> lk(m);
      if (!why.empty()) bad[i] = why;
      slot_frame[slot_of(i)] = i;
    }
    cv.notify_all();
  }

  // reader thread of a JPEG source: pread the compressed bytes, entropy-decode into the pinned slot
  void read_jpeg_loop() {
    std::vector<uint8_t> own;
    for (;;) {
      int64_t i;
      {
        std::unique_lock<std::mutex> lk(m);
        if (stop || next_read >= n_frames) return;
        i = next_read++;
        cv.wait(lk, [&] { return stop || i / B < released + ring; });
        if (stop) return;
      }
      const size_t len = (size_t)lengths[(size_t)i];
      std::vector<uint8_t>& buf = (entropy || restart) ? slot_src[slot_of(i)] : own;   // the GPU route keeps the bytes with the slot
      buf.resize(len);
      std::string why;
      size_t got = 0;
      int d = one_fd;
      if (d < 0) {
        const std::string& p = paths[(size_t)file_index[(size_t)i]];
        d = ::open(p.c_str(), O_RDONLY | O_CLOEXEC);
        if (d < 0) why = "frame " + std::to_string(i) + ": cannot open '" + p + "': " + strerror(errno);
      }
      while (why.empty() && got < len) {
        const ssize_t r = ::pread(d, buf.data() + got, len - got, (off_t)(offsets[(size_t)i] + (int64_t)got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          why = "frame " + std::to_string(i) + " could not be read (" + (r == 0 ? std::string("file ends early") : std::string(strerror(errno))) + ")";
          break;
        }
        got += (size_t)r;
      }
      if (d >= 0 && d != one_fd) ::close(d);
      if (why.empty()) fill_slot(i, buf.data(), len, why);
      publish(i, why);
    }
  }

  // reader thread: frames in file order, each into the pinned slot of its (batch, position)
  void read_loop() {
    for (;;) {
      int64_t i;
      {
        std::unique_lock<std::mutex> lk(m);
        if (stop || next_read >= n_frames) return;
        i = next_read++;
        cv.wait(lk, [&] { return stop || i / B < released + ring; });
        if (stop) return;
      }
      uint8_t* dst = pinned + slot_of(i) * src_bytes;
      size_t got = 0;
      if (!mem.empty()) {                       // memory mode: one copy into the pinned slot, like the page-cache copy of a pread
        memcpy(dst, mem[(size_t)i], src_bytes);
        got = src_bytes;
      }
      while (got < src_bytes) {
        const ssize_t r = ::pread(fd, dst + got, src_bytes - got, (off_t)(offsets[(size_t)i] + (int64_t)got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          set_error("frame " + std::to_string(i) + " could not be read (" + (r == 0 ? std::string("file ends early") : std::string(strerror(errno))) + ")");
          return;
        }
        got += (size_t)r;
      }
      {
        std::lock_guard<std::mutex> lk(m);
        slot_frame[slot_of(i)] = i;
      }
      cv.notify_all();
    }
  }

  // next() on the GPU entropy route, batch j of `count` frames: waits for the batch's event, then has the host parser decode every
  // frame whose status word is not 0 (not converged and invalid alike) from the bytes kept with its slot: parse() + check_record,
  // upload, the two pixel kernels, a wait. A frame the parser refuses too throws its message, as the host route reports it.
  void settle_batch(int64_t j, int count) {
    GTX_HIP(hipSetDevice(ctx.device));
    GTX_HIP(hipEventSynchronize(ev[(size_t)(j % ring)]));
    bool again = false;
    for (int k = 0; k < count; ++k) {
      const int64_t i = j * B + k;
      const size_t s = slot_of(i);
      const int tag = slot_tag[s];
      if (tag == 3) {                                           // the restart route handed it back to its reader thread
        ++rstats[1];
        continue;
      }
      if (tag == 0) {                                           // the reader thread decoded it: plan() handed it back (or the host route is on)
        if (entropy) ++stats[1];
        continue;
      }
      if ((tag == 2 ? h_rstatus[s] : h_status[2 * s]) == 0) {
        ++(tag == 2 ? rstats[0] : stats[0]);
        continue;
      }
      std::string why;
      slot_tag[s] = 0;
      if (!decode_into_slot(i, slot_src[s].data(), slot_src[s].size(), why)) {
        set_error(why);
        gtx::fail(GTX_ERR_INTERNAL, "%s", why.c_str());
      }
      ++(tag == 2 ? rstats[2] : stats[2]);
      if (!fb_rec.p) fb_rec.alloc(src_bytes), fb_planes.alloc(64 * gtx::jpeg::max_blocks(h, w));
      gtx::jpeg::RecordHeader hd;
      memcpy(&hd, pinned + s * src_bytes, sizeof hd);
      GTX_HIP(hipStreamSynchronize(ctx.stream));               // fb_rec may still be read by the frame before
      GTX_HIP(hipMemcpyAsync(fb_rec.p, pinned + s * src_bytes, slot_len[s], hipMemcpyHostToDevice, ctx.stream));
      gtx::jpeg_decode_launch(&ctx, fb_rec.p, hd, fb_planes.p, dev.as<uint8_t>() + s * bgr_bytes);
      again = true;
    }
    if (again) GTX_HIP(hipStreamSynchronize(ctx.stream));
  }

  // uploader thread: slots in frame order onto the copy stream, one event per batch (a shorter last batch gets its event
  // when the end of the source is known)
  void upload_loop() {
    if (hipSetDevice(ctx.device) != hipSuccess) return set_error("hipSetDevice failed on the feeder's upload thread");
    std::vector<int64_t> pending;                               // the batch's frames on the restart-interval route
    std::vector<const uint8_t*> rs_plans;
    std::vector<uint8_t*> rs_recs;
    std::vector<gtx::jpeg::PlanHeader> rs_phs;
    try {
      for (int64_t i = 0;; ++i) {
        bool end;
        {
          std::unique_lock<std::mutex> lk(m);
          cv.wait(lk, [&] { return stop || (n_frames >= 0 && i >= n_frames) || slot_frame[slot_of(i)] == i; });
          if (stop) return;
          end = n_frames >= 0 && i >= n_frames;
        }
        if (end && i % B == 0) return;
        if (!end && kind == 2) {
          std::string why;
          {
            std::lock_guard<std::mutex> lk(m);
            auto it = bad.find(i);
            if (it != bad.end()) why = it->second;
          }
          if (!why.empty()) return set_error(why);            // every batch before this frame's has its event already
        }
        if (!end) {
          const size_t s = slot_of(i);
          uint8_t* bgr = dev.as<uint8_t>() + s * bgr_bytes;
          if (kind == 2 && restart && slot_tag[s] == 2) {       // decoded with the rest of its batch, below
            const size_t k = (size_t)(i % B);
            GTX_HIP(hipMemcpyAsync(rs_plan.as<uint8_t>() + k * src_bytes, pinned + s * src_bytes, slot_len[s], hipMemcpyHostToDevice, ctx.stream));
            pending.push_back(i);
          } else if (kind == 2 && entropy && slot_tag[s] == 1) {
            gtx::jpeg::PlanHeader ph;
            memcpy(&ph, pinned + s * src_bytes, sizeof ph);
            GTX_HIP(hipMemcpyAsync(dev_plan.p, pinned + s * src_bytes, slot_len[s], hipMemcpyHostToDevice, ctx.stream));   // the plan at its real length
            entropy->enqueue(dev_plan.as<const uint8_t>(), ph, 0, 0, dev_rec.as<uint8_t>());
            gtx::jpeg_decode_launch(&ctx, dev_rec.p, gtx::JpegEntropy::record_header(ph), dev_planes.p, bgr);
            GTX_HIP(hipMemcpyAsync(h_status + 2 * s, entropy->d_result(), 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, ctx.stream));
          } else if (kind == 2) {
            gtx::jpeg::RecordHeader hd;
            memcpy(&hd, pinned + s * src_bytes, sizeof hd);
            GTX_HIP(hipMemcpyAsync(dev_rec.p, pinned + s * src_bytes, slot_len[s], hipMemcpyHostToDevice, ctx.stream));
            gtx::jpeg_decode_launch(&ctx, dev_rec.p, hd, dev_planes.p, bgr);
          } else if (kind == 1) {
            uint8_t* yuv = dev_yuv.as<uint8_t>() + s * src_bytes;
            GTX_HIP(hipMemcpyAsync(yuv, pinned + s * src_bytes, src_bytes, hipMemcpyHostToDevice, ctx.stream));
            gtx::yuv420_to_bgr_dev(&ctx, yuv, h, w, bgr);
          } else {
            GTX_HIP(hipMemcpyAsync(bgr, pinned + s * src_bytes, src_bytes, hipMemcpyHostToDevice, ctx.stream));
          }
        }
        if (end || i % B == B - 1) {
          const int64_t j = end ? (i - 1) / B : i / B;
          if (!pending.empty()) {                                // every interval of the batch's restart frames in one launch
            rs_plans.clear(), rs_recs.clear(), rs_phs.clear();
            for (const int64_t fi : pending) {
              const size_t k = (size_t)(fi % B);
              gtx::jpeg::PlanHeader ph;
              memcpy(&ph, pinned + slot_of(fi) * src_bytes, sizeof ph);
              rs_plans.push_back(rs_plan.as<const uint8_t>() + k * src_bytes), rs_recs.push_back(rs_rec.as<uint8_t>() + k * src_bytes), rs_phs.push_back(ph);
            }
            restart->enqueue((int)pending.size(), rs_plans.data(), rs_phs.data(), rs_recs.data());
            for (size_t q = 0; q < pending.size(); ++q) {
              const size_t fs = slot_of(pending[q]);
              gtx::jpeg_decode_launch(&ctx, rs_recs[q], gtx::JpegEntropy::record_header(rs_phs[q]), dev_planes.p, dev.as<uint8_t>() + fs * bgr_bytes);
              GTX_HIP(hipMemcpyAsync(h_rstatus + fs, restart->d_result((int)q), sizeof(uint32_t), hipMemcpyDeviceToHost, ctx.stream));
            }
            pending.clear();
          }
          GTX_HIP(hipEventRecord(ev[(size_t)(j % ring)], ctx.stream));
          {
            std::lock_guard<std::mutex> lk(m);
            issued = j + 1;
          }
          cv.notify_all();
          if (end) return;
        }
      }
    } catch (const std::exception& e) {
      set_error(e.what());
    }
  }
};

using gtx::guarded;

extern "C" {

namespace {
void feeder_create(int device, hipStream_t borrowed, int h, int w, int kind, int batch, int ring, gtx_feeder** out) {
  if (!out) gtx::fail(GTX_ERR_INVALID, "out is NULL");
  if (h <= 0 || w <= 0 || kind < 0 || kind > 2 || batch < 1 || ring < 2)
    gtx::fail(GTX_ERR_INVALID, "feeder: bad geometry (h %d, w %d, kind %d, batch %d, ring %d)", h, w, kind, batch, ring);
  GTX_HIP(hipSetDevice(device));
  std::unique_ptr<gtx_feeder> f(new gtx_feeder);
  f->ctx.device = device;
  f->h = h, f->w = w, f->kind = kind, f->B = batch, f->ring = ring;
  f->bgr_bytes = (size_t)h * w * 3;
  f->src_bytes = kind == 1 ? (size_t)h * w + 2 * (size_t)((h + 1) / 2) * ((w + 1) / 2) : f->bgr_bytes;
  if (kind == 2) {
    if (h > gtx::jpeg::kMaxDim || w > gtx::jpeg::kMaxDim) gtx::fail(GTX_ERR_UNSUPPORTED, "feeder: JPEG frames larger than %d are not decoded", gtx::jpeg::kMaxDim);
    f->src_bytes = (gtx::jpeg::record_bound(h, w) + 63) / 64 * 64;     // the worst-case record: every block 64 coefficients long
  }
  if (borrowed) {
    f->ctx.stream = borrowed;
    f->own_stream = false;
  } else {
    GTX_HIP(hipStreamCreateWithFlags(&f->ctx.stream, hipStreamNonBlocking));
  }
  const size_t slots = (size_t)ring * batch;
  GTX_HIP(hipHostMalloc((void**)&f->pinned, slots * f->src_bytes, hipHostMallocDefault));
  f->dev.alloc(slots * f->bgr_bytes);
  if (kind == 1) f->dev_yuv.alloc(slots * f->src_bytes);
  if (kind == 2) {
    f->dev_rec.alloc(f->src_bytes);
    f->dev_planes.alloc(64 * gtx::jpeg::max_blocks(h, w));
    f->slot_len.assign(slots, 0);
  }
  f->ev.resize((size_t)ring);
  for (auto& e : f->ev) GTX_HIP(hipEventCreateWithFlags(&e, gtx::wait_event_flags(false)));
  f->slot_frame.assign(slots, -1);
  *out = f.release();
}
}  // namespace

int gtx_feeder_create(int device, int h, int w, int kind, int batch, int ring, gtx_feeder** out) {
  return guarded([&] { feeder_create(device, nullptr, h, w, kind, batch, ring, out); });
}

int gtx_feeder_create_on(gtx_ctx* copy_ctx, int h, int w, int kind, int batch, int ring, gtx_feeder** out) {
  return guarded([&] {
    if (!copy_ctx) gtx::fail(GTX_ERR_INVALID, "copy_ctx is NULL");
    feeder_create(copy_ctx->device, copy_ctx->stream, h, w, kind, batch, ring, out);
  });
}

void gtx_feeder_destroy(gtx_feeder* f) { delete f; }

int gtx_feeder_open_file(gtx_feeder* f, const char* path, const int64_t* offsets, int64_t n_frames, int n_threads) {
  return guarded([&] {
    if (!f || !path || (n_frames > 0 && !offsets)) gtx::fail(GTX_ERR_INVALID, "feeder_open_file: NULL argument");
    if (f->fd >= 0 || f->uploader.joinable()) gtx::fail(GTX_ERR_STATE, "feeder already has a source");
    if (f->kind == 2) gtx::fail(GTX_ERR_INVALID, "feeder_open_file: a JPEG feeder is opened with gtx_feeder_open_jpeg");
    f->fd = ::open(path, O_RDONLY | O_CLOEXEC);
    if (f->fd < 0) gtx::fail(GTX_ERR_INVALID, "feeder: cannot open '%s': %s", path, strerror(errno));
    f->offsets.assign(offsets, offsets + n_frames);
    f->n_frames = n_frames;
    f->uploader = std::thread([f] { f->upload_loop(); });
    for (int t = 0; t < std::max(1, std::min(n_threads, 16)); ++t) f->readers.emplace_back([f] { f->read_loop(); });
  });
}

int gtx_feeder_open_memory(gtx_feeder* f, const void* const* frames, int64_t n_frames, int n_threads) {
  return guarded([&] {
    if (!f || (n_frames > 0 && !frames)) gtx::fail(GTX_ERR_INVALID, "feeder_open_memory: NULL argument");
    if (f->fd >= 0 || f->uploader.joinable()) gtx::fail(GTX_ERR_STATE, "feeder already has a source");
    if (f->kind == 2) gtx::fail(GTX_ERR_INVALID, "feeder_open_memory: a JPEG feeder is opened with gtx_feeder_open_jpeg or fed by gtx_feeder_push");
    for (int64_t i = 0; i < n_frames; ++i) {
      if (!frames[i]) gtx::fail(GTX_ERR_INVALID, "feeder_open_memory: frame %lld is NULL", (long long)i);
      f->mem.push_back(static_cast<const uint8_t*>(frames[i]));
    }
    f->n_frames = n_frames;
    f->uploader = std::thread([f] { f->upload_loop(); });
    for (int t = 0; t < std::max(1, std::min(n_threads, 16)); ++t) f->readers.emplace_back([f] { f->read_loop(); });
  });
}

int gtx_feeder_open_jpeg(gtx_feeder* f, const char* const* paths, int n_paths, const int32_t* file_index, const int64_t* offsets,
                         const int64_t* lengths, int64_t n_frames, int n_threads) {
  return guarded([&] {
    if (!f || n_frames < 0 || n_paths < 0 || (n_frames > 0 && (!paths || !file_index || !offsets || !lengths)))
      gtx::fail(GTX_ERR_INVALID, "feeder_open_jpeg: NULL argument");
    if (f->kind != 2) gtx::fail(GTX_ERR_INVALID, "feeder_open_jpeg: the feeder was created with kind %d, not 2", f->kind);
    if (f->fd >= 0 || f->one_fd >= 0 || !f->paths.empty() || f->uploader.joinable()) gtx::fail(GTX_ERR_STATE, "feeder already has a source");
    for (int64_t i = 0; i < n_frames; ++i) {
      if (file_index[i] < 0 || file_index[i] >= n_paths) gtx::fail(GTX_ERR_INVALID, "feeder_open_jpeg: frame %lld names file %d of %d", (long long)i, file_index[i], n_paths);
      if (offsets[i] < 0 || lengths[i] < 4 || lengths[i] > (int64_t)1 << 30)
        gtx::fail(GTX_ERR_INVALID, "feeder_open_jpeg: frame %lld has %lld bytes at offset %lld", (long long)i, (long long)lengths[i], (long long)offsets[i]);
    }
    std::vector<char> named((size_t)n_paths, 0);                // only the files the (possibly sliced) index names are touched
    for (int64_t i = 0; i < n_frames; ++i) named[(size_t)file_index[i]] = 1;
    f->paths.assign((size_t)n_paths, std::string());
    int n_named = 0, only = -1;
    for (int k = 0; k < n_paths; ++k) {
      if (!named[(size_t)k]) continue;
      if (!paths[k]) gtx::fail(GTX_ERR_INVALID, "feeder_open_jpeg: path %d is NULL", k);
      f->paths[(size_t)k] = paths[k];
      ++n_named, only = k;
    }
    if (n_named == 1) {                                          // a clip: one descriptor for the feeder's lifetime
      f->one_fd = ::open(f->paths[(size_t)only].c_str(), O_RDONLY | O_CLOEXEC);
      if (f->one_fd < 0) gtx::fail(GTX_ERR_INVALID, "feeder: cannot open '%s': %s", f->paths[(size_t)only].c_str(), strerror(errno));
    } else if (n_frames > 0) {                                   // a file per frame: a missing first file is reported here, like a missing clip
      const std::string& p = f->paths[(size_t)file_index[0]];
      if (::access(p.c_str(), R_OK) != 0) gtx::fail(GTX_ERR_INVALID, "feeder: cannot open '%s': %s", p.c_str(), strerror(errno));
    }
    f->file_index.assign(file_index, file_index + n_frames);
    f->offsets.assign(offsets, offsets + n_frames);
    f->lengths.assign(lengths, lengths + n_frames);
    f->n_frames = n_frames;
    f->uploader = std::thread([f] { f->upload_loop(); });
    for (int t = 0; t < std::max(1, std::min(n_threads, 16)); ++t) f->readers.emplace_back([f] { f->read_jpeg_loop(); });
  });
}

int gtx_feeder_set_jpeg_entropy(gtx_feeder* f, int gpu) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_entropy: feeder is NULL");
    if (f->kind != 2) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_entropy: the feeder was created with kind %d, not 2", f->kind);
    if (f->fd >= 0 || f->one_fd >= 0 || !f->paths.empty() || f->uploader.joinable()) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_entropy: the feeder already has a source");
    if (!gpu) {
      f->entropy.reset();
      return;
    }
    if (f->entropy) return;
    GTX_HIP(hipSetDevice(f->ctx.device));
    const size_t slots = (size_t)f->ring * f->B;
    if (!f->h_status) GTX_HIP(hipHostMalloc((void**)&f->h_status, slots * 2 * sizeof(uint32_t), hipHostMallocDefault));
    f->dev_plan.alloc(f->src_bytes);
    f->slot_tag.assign(slots, 0);
    f->slot_src.assign(slots, std::vector<uint8_t>());
    f->entropy.reset(new gtx::JpegEntropy(&f->ctx, gtx::jpeg::max_blocks(f->h, f->w), f->src_bytes > gtx::jpeg::kPlanStreamOffset ? f->src_bytes - gtx::jpeg::kPlanStreamOffset : 4,   // (a smaller slot holds no plan)
                                             gtx::kJpegEntropySubBits));
  });
}

int gtx_feeder_set_jpeg_restart(gtx_feeder* f, int on) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_restart: feeder is NULL");
    if (f->kind != 2) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_restart: the feeder was created with kind %d, not 2", f->kind);
    if (f->fd >= 0 || f->one_fd >= 0 || !f->paths.empty() || f->uploader.joinable()) gtx::fail(GTX_ERR_INVALID, "feeder_set_jpeg_restart: the feeder already has a source");
    if (!on) {
      f->restart.reset();
      return;
    }
    if (f->restart) return;
    GTX_HIP(hipSetDevice(f->ctx.device));
    const size_t slots = (size_t)f->ring * f->B;
    if (!f->h_rstatus) GTX_HIP(hipHostMalloc((void**)&f->h_rstatus, slots * sizeof(uint32_t), hipHostMallocDefault));
    f->rs_plan.alloc((size_t)f->B * f->src_bytes);
    f->rs_rec.alloc((size_t)f->B * f->src_bytes);
    if (f->slot_tag.size() != slots) f->slot_tag.assign(slots, 0);
    if (f->slot_src.size() != slots) f->slot_src.assign(slots, std::vector<uint8_t>());
    f->restart.reset(new gtx::JpegRestart(&f->ctx, f->B, gtx::jpeg::max_blocks(f->h, f->w)));
  });
}

int gtx_feeder_jpeg_restart_stats(gtx_feeder* f, int64_t out[3]) {
  return guarded([&] {
    if (!f || !out) gtx::fail(GTX_ERR_INVALID, "feeder_jpeg_restart_stats: NULL argument");
    for (int k = 0; k < 3; ++k) out[k] = f->rstats[k].load();
  });
}

int gtx_feeder_jpeg_stats(gtx_feeder* f, int64_t out[3]) {
  return guarded([&] {
    if (!f || !out) gtx::fail(GTX_ERR_INVALID, "feeder_jpeg_stats: NULL argument");
    for (int k = 0; k < 3; ++k) out[k] = f->stats[k].load();
  });
}

int gtx_feeder_open_push(gtx_feeder* f) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder is NULL");
    if (f->fd >= 0 || f->uploader.joinable()) gtx::fail(GTX_ERR_STATE, "feeder already has a source");
    f->uploader = std::thread([f] { f->upload_loop(); });
  });
}

int gtx_feeder_push(gtx_feeder* f, const void* frame, size_t bytes) {
  return guarded([&] {
    if (!f || !frame) gtx::fail(GTX_ERR_INVALID, "feeder_push: NULL argument");
    if (f->kind != 2 && bytes != f->src_bytes) gtx::fail(GTX_ERR_INVALID, "feeder_push: frame has %zu bytes, the feeder was built for %zu", bytes, f->src_bytes);
    int64_t i;
    {
      std::unique_lock<std::mutex> lk(f->m);
      if (f->n_frames >= 0) gtx::fail(GTX_ERR_STATE, "feeder_push after feeder_finish");
      i = f->next_read;
      f->cv.wait(lk, [&] { return f->stop || i / f->B < f->released + f->ring; });
      if (f->stop) gtx::fail(GTX_ERR_STATE, "feeder stopped: %s", f->error.c_str());
      f->next_read = i + 1;
    }
    if (f->kind == 2) {                                  // a compressed frame: decoded here, on the producer's thread
      std::string why;
      f->fill_slot(i, static_cast<const uint8_t*>(frame), bytes, why);
      f->publish(i, why);
      if (!why.empty()) gtx::fail(GTX_ERR_INVALID, "%s", why.c_str());
      return;
    }
    memcpy(f->pinned + f->slot_of(i) * f->src_bytes, frame, bytes);
    {
      std::lock_guard<std::mutex> lk(f->m);
      f->slot_frame[f->slot_of(i)] = i;
    }
    f->cv.notify_all();
  });
}

int gtx_feeder_push_at(gtx_feeder* f, int64_t i, const void* frame, size_t bytes) {
  return guarded([&] {
    if (!f || !frame || i < 0) gtx::fail(GTX_ERR_INVALID, "feeder_push_at: bad argument");
    if (f->kind != 2 && bytes != f->src_bytes) gtx::fail(GTX_ERR_INVALID, "feeder_push_at: frame has %zu bytes, the feeder was built for %zu", bytes, f->src_bytes);
    {
      std::unique_lock<std::mutex> lk(f->m);
      if (f->n_frames >= 0) gtx::fail(GTX_ERR_STATE, "feeder_push_at after feeder_finish");
      f->cv.wait(lk, [&] { return f->stop || i / f->B < f->released + f->ring; });
      if (f->stop) gtx::fail(GTX_ERR_STATE, "feeder stopped: %s", f->error.c_str());
      if (i / f->B < f->released) gtx::fail(GTX_ERR_STATE, "feeder_push_at: frame %lld belongs to a batch that was already consumed", (long long)i);
    }
    if (f->kind == 2) {
      std::string why;
      f->fill_slot(i, static_cast<const uint8_t*>(frame), bytes, why);
      {
        std::lock_guard<std::mutex> lk(f->m);
        if (i + 1 > f->next_read) f->next_read = i + 1;
      }
      f->publish(i, why);
      if (!why.empty()) gtx::fail(GTX_ERR_INVALID, "%s", why.c_str());
      return;
    }
    memcpy(f->pinned + f->slot_of(i) * f->src_bytes, frame, bytes);
    {
      std::lock_guard<std::mutex> lk(f->m);
      f->slot_frame[f->slot_of(i)] = i;
      if (i + 1 > f->next_read) f->next_read = i + 1;
    }
    f->cv.notify_all();
  });
}

int gtx_feeder_finish(gtx_feeder* f) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder is NULL");
    {
      std::lock_guard<std::mutex> lk(f->m);
      if (f->n_frames < 0) f->n_frames = f->next_read;
    }
    f->cv.notify_all();
  });
}

int gtx_feeder_stop(gtx_feeder* f) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder is NULL");
    {
      std::lock_guard<std::mutex> lk(f->m);
      if (f->error.empty()) f->error = "the feeder was stopped";
      f->stop = true;
    }
    f->cv.notify_all();
  });
}

int gtx_feeder_next(gtx_feeder* f, void** dptr, int* n, int64_t* batch_index) {
  return guarded([&] {
    if (!f || !dptr || !n) gtx::fail(GTX_ERR_INVALID, "feeder_next: NULL argument");
    std::unique_lock<std::mutex> lk(f->m);
    f->cv.wait(lk, [&] { return !f->error.empty() || f->issued > f->handed || (f->n_frames >= 0 && f->handed >= f->n_batches()); });
    if (f->issued > f->handed && (f->dead_from < 0 || f->handed < f->dead_from)) {   // batches that arrived before a failure are still delivered
      const int64_t j = f->handed;
      const int count = (int)((f->n_frames >= 0 && (j + 1) * f->B > f->n_frames) ? f->n_frames - j * f->B : f->B);
      if (f->entropy || f->restart) {                  // a GPU entropy route: the batch's status words decide who decoded it
        lk.unlock();
        try {
          f->settle_batch(j, count);
        } catch (const std::exception& e) {               // the parser's refusal or a HIP failure: every later call reports it too
          f->set_error(e.what());
          lk.lock();
          f->dead_from = j;
          throw;
        }
        lk.lock();
      }
      f->handed = j + 1;
      *dptr = f->dev.as<uint8_t>() + (size_t)(j % f->ring) * f->B * f->bgr_bytes;
      *n = count;
      if (batch_index) *batch_index = j;
      return;
    }
    if (!f->error.empty()) gtx::fail(GTX_ERR_INTERNAL, "%s", f->error.c_str());
    *dptr = nullptr;
    *n = 0;
    if (batch_index) *batch_index = f->handed;
  });
}

int gtx_feeder_wait(gtx_feeder* f, int64_t batch_index, gtx_ctx* consumer) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder is NULL");
    hipEvent_t e;
    {
      std::lock_guard<std::mutex> lk(f->m);
      if (batch_index < 0 || batch_index >= f->issued || batch_index < f->released)
        gtx::fail(GTX_ERR_STATE, "feeder_wait: batch %lld is not resident (issued %lld, released %lld)", (long long)batch_index, (long long)f->issued, (long long)f->released);
      e = f->ev[(size_t)(batch_index % f->ring)];
    }
    GTX_HIP(hipSetDevice(f->ctx.device));
    if (consumer) GTX_HIP(hipStreamWaitEvent(consumer->stream, e, 0));
    else GTX_HIP(hipEventSynchronize(e));
  });
}

int gtx_feeder_release(gtx_feeder* f, int64_t n_batches) {
  return guarded([&] {
    if (!f) gtx::fail(GTX_ERR_INVALID, "feeder is NULL");
    {
      std::lock_guard<std::mutex> lk(f->m);
      if (n_batches > f->handed) gtx::fail(GTX_ERR_STATE, "feeder_release(%lld): only %lld batches were handed out", (long long)n_batches, (long long)f->handed);
      if (n_batches > f->released) f->released = n_batches;
    }
    f->cv.notify_all();
  });
}

}  // extern "C"
