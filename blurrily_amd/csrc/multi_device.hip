// multi_device.hip -- option "devices" > 1: replicas of the device images and a batch sharded over them.
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

namespace blurrily {
namespace detail {

// ---- "devices" > 1: the batch sharded over replicas of the device image, in ONE process -----------------------
// (the drop-in host is a single process: the reference's server is one reactor, lib/blurrily/server.rb:19-30,
// its glue one call at a time, ext/blurrily/map_ext.c:131-162 -- SURVEY.md section 8(e)'s partition, replicate and
// shard contiguously, behind the C ABI instead of behind torch.distributed)

// (on its device, its stream idle: then the side map and the replica give back what they hold)
void free_replica(Replica& r) {
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (r.device >= 0) (void)hipSetDevice(r.device);
  if (r.stream) (void)hipStreamSynchronize(r.stream);
  if (r.side) {
    trigram_map s = r.side;
    if (s->dev.device >= 0) device_index_free(&s->dev);
    if (s->delta.device >= 0) device_index_free(&s->delta);
    delete s;
  }
  r = Replica();
  if (prev >= 0) (void)hipSetDevice(prev);
}

// Bring the replicas up to date with the primary's images (which ensure_device has just brought up to date with
// the host index): device-to-device clones of whatever changed -- the base image after a rebuild, the delta image
// when the set of pending puts changed, the tombstone bitmap and the bucket totals when anything was logged.
static int ensure_replicas(trigram_map m) {
  int ndev = 0;
  BLURRILY_HIP_TRY(hipGetDeviceCount(&ndev));
  const size_t want = m->n_devices > 1 ? m->n_devices - 1 : 0;
  while (m->replicas.size() > want) { free_replica(m->replicas.back()); m->replicas.pop_back(); }
  while (m->replicas.size() < want) {
    Replica r;
    // replica k lives on the k-th device behind the primary's, round the visible ones (more replicas than devices --
    // the tests' way of running the multi-device path on one GPU -- share devices)
    r.device = (m->dev.device + 1 + int(m->replicas.size())) % ndev;
    r.side = new (std::nothrow) trigram_map_t();
    if (!r.side) { errno = ENOMEM; return -1; }
    r.side->mirror_of = m;
    // The shard's needles reach the replica, and its rows the caller's buffers, by hipMemcpyPeerAsync.  With peer
    // access enabled BOTH ways those copies are the devices' own, point to point (xGMI on an MI355X node); without it
    // the runtime stages them through host memory -- same rows, and said so once on stderr, since that is not the
    // gather SURVEY.md section 8(e) describes.
    r.same_device = r.device == m->dev.device;
    if (!r.same_device) {
      int to = 0, from = 0;
      const bool can = hipDeviceCanAccessPeer(&to, m->dev.device, r.device) == hipSuccess && to &&
                       hipDeviceCanAccessPeer(&from, r.device, m->dev.device) == hipSuccess && from;
      bool on_ = can;
      if (can) {
        for (int pass = 0; pass < 2 && on_; ++pass) {
          DeviceScope here(pass ? r.device : m->dev.device);
          const hipError_t e = hipDeviceEnablePeerAccess(pass ? m->dev.device : r.device, 0);
          if (e == hipErrorPeerAccessAlreadyEnabled) (void)hipGetLastError();
          else if (e != hipSuccess) on_ = false;
        }
      }
      r.peer_access = on_;
      if (!on_)
        std::fprintf(stderr, "blurrily_hip: no peer access between device %d and device %d (%s): the rows of that replica "
                             "travel through host memory\n", m->dev.device, r.device, can ? "enabling it failed" : "not offered");
    }
    DeviceScope on(r.device);
    if (r.stream.make() < 0 || r.ev_done.make(hipEventDisableTiming) < 0 || r.ev_t.make() < 0) {
      free_replica(r);
      errno = EIO;
      return -1;
    }
    m->replicas.push_back(std::move(r));
  }
  if (m->ev_ready.make(hipEventDisableTiming) < 0 || m->ev_t.make() < 0) return -1;
  for (Replica& r : m->replicas) {
    trigram_map s = r.side;
    // the sweep's settings and the measured choices follow the primary's: its choice where it has one -- and, after a
    // clone, only those
    s->sweep = m->sweep;
    s->n_cus = 0;
    if (r.base_builds != m->base_builds || s->dev.device < 0) {
      if (device_index_clone(m->dev, r.device, &s->dev) < 0) return -1;
      forget_choices(s);
      r.base_builds = m->base_builds;
      r.log_version = ~0ull;                                   // (tombstones and totals below)
      r.delta_image_version = ~0ull;
    }
    for (int c = 0; c < 8; ++c) if (m->cls[c].choice) s->cls[c].choice = m->cls[c].choice;
    if (s->n_cus == 0) {
      hipDeviceProp_t prop;
      BLURRILY_HIP_TRY(hipGetDeviceProperties(&prop, r.device));
      s->n_cus = prop.multiProcessorCount;
    }
    if (r.delta_image_version != m->delta_image_version) {
      if (m->delta.device < 0) { if (s->delta.device >= 0) device_index_free(&s->delta); }
      else if (device_index_clone(m->delta, r.device, &s->delta) < 0) return -1;
      r.delta_image_version = m->delta_image_version;
    }
    if (r.log_version != m->log_version) {
      DeviceScope on(r.device);
      BLURRILY_HIP_TRY(hipMemcpyPeer(s->dev.d_tomb, r.device, m->dev.d_tomb, m->dev.device,
                                     ((size_t(m->dev.n_refs) + 31) / 32 + 1) * sizeof(uint32_t)));
      if (m->d_code_total_now) {
        if (s->d_code_total_now.alloc(kNumCodes) < 0) return -1;
        BLURRILY_HIP_TRY(hipMemcpyPeer(s->d_code_total_now, r.device, m->d_code_total_now, m->dev.device,
                                       kNumCodes * sizeof(uint32_t)));
      }
      r.log_version = m->log_version;
    }
  }
  return 0;
}

// n device-resident needles on the primary's device, results into buffers there, the work sharded contiguously over
// the primary and its replicas: every replica gets the batch's needles by ONE peer copy, searches its shard on its own
// stream and sends its block of rows (and counts, nb_entries) straight into the caller's buffers by peer copies --
// the gather of SURVEY.md section 8(e), point to point over xGMI.  Everything is enqueued: `stream` waits for the
// replicas' events, the host for nothing (timing mode apart).
static int run_find_multi_enqueue(trigram_map m, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n,
                           uint16_t limit, trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, hipStream_t stream) {
  if (apply_tombstones(m, stream) < 0) return -1;             // (the bits are set before the replicas copy the bitmap)
  if (ensure_replicas(m) < 0) return -1;
  const size_t R = m->replicas.size() + 1;
  const int P = m->dev.device;
  BLURRILY_HIP_TRY(hipEventRecord(m->ev_ready[0], stream));      // the caller's needles are in place behind this
  const bool timing = m->timing;
  auto bound = [&](size_t r) { return n * r / R; };
  const size_t off_bytes = align_up((n + 1) * sizeof(uint64_t), 256);
  for (size_t k = 0; k + 1 < R; ++k) {
    Replica& r = m->replicas[k];
    const size_t a = bound(k + 1), b = bound(k + 2), c = b - a;
    if (c == 0) continue;
    DeviceScope on(r.device);
    const size_t cnt_bytes = align_up(c * sizeof(uint32_t), 256);
    const size_t row_bytes = align_up(std::max<size_t>(c * size_t(limit) * sizeof(trigram_match_t), 16), 256);
    if (r.d_in.reserve(off_bytes + std::max<size_t>(packed_bytes, 16), r.stream) < 0 ||
        r.d_out.reserve(row_bytes + 2 * cnt_bytes, r.stream) < 0)
      return -1;
    unsigned char* in = static_cast<unsigned char*>(r.d_in.p);
    unsigned char* out = static_cast<unsigned char*>(r.d_out.p);
    BLURRILY_HIP_TRY(hipStreamWaitEvent(r.stream, m->ev_ready[0], 0));
    BLURRILY_HIP_TRY(hipMemcpyPeerAsync(in, r.device, d_offsets, P, (n + 1) * sizeof(uint64_t), r.stream));
    if (packed_bytes)
      BLURRILY_HIP_TRY(hipMemcpyPeerAsync(in + off_bytes, r.device, d_packed, P, packed_bytes, r.stream));
    trigram_match rows = reinterpret_cast<trigram_match>(out);
    uint32_t* counts = reinterpret_cast<uint32_t*>(out + row_bytes);
    uint32_t* nb = reinterpret_cast<uint32_t*>(out + row_bytes + cnt_bytes);
    r.side->timing = false;
    r.side->collect_stats = false;
    if (timing) BLURRILY_HIP_TRY(hipEventRecord(r.ev_t[0], r.stream));
    // (the shard's offsets are the batch's own, from its first needle on: they index the whole needle buffer)
    if (run_find(r.side, reinterpret_cast<const char*>(in + off_bytes), packed_bytes,
                 reinterpret_cast<const uint64_t*>(in) + a, c, limit, rows, counts, d_nb ? nb : nullptr, true, true,
                 r.stream) < 0)
      return -1;
    if (timing) BLURRILY_HIP_TRY(hipEventRecord(r.ev_t[1], r.stream));
    if (limit)
      BLURRILY_HIP_TRY(hipMemcpyPeerAsync(d_results + a * size_t(limit), P, rows, r.device,
                                          c * size_t(limit) * sizeof(trigram_match_t), r.stream));
    BLURRILY_HIP_TRY(hipMemcpyPeerAsync(d_counts + a, P, counts, r.device, c * sizeof(uint32_t), r.stream));
    if (d_nb) BLURRILY_HIP_TRY(hipMemcpyPeerAsync(d_nb + a, P, nb, r.device, c * sizeof(uint32_t), r.stream));
    BLURRILY_HIP_TRY(hipEventRecord(r.ev_done[0], r.stream));
  }
  // the primary's own shard, on the caller's stream (its timing mode would wait for it: the replicas are under way)
  const size_t c0 = bound(1);
  m->timing = false;
  if (timing) BLURRILY_HIP_TRY(hipEventRecord(m->ev_t[0], stream));
  const int rc = run_find(m, d_packed, packed_bytes, d_offsets, c0, limit, d_results, d_counts, d_nb, true, true, stream);
  m->timing = timing;
  if (rc < 0) return -1;
  if (timing) BLURRILY_HIP_TRY(hipEventRecord(m->ev_t[1], stream));
  for (size_t k = 0; k + 1 < R; ++k)
    if (bound(k + 2) > bound(k + 1)) BLURRILY_HIP_TRY(hipStreamWaitEvent(stream, m->replicas[k].ev_done[0], 0));
  if (timing) {                                               // last_find_kernel_ms: the slowest shard's search
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
    float ms = 0.f, worst = 0.f;
    BLURRILY_HIP_TRY(hipEventElapsedTime(&worst, m->ev_t[0], m->ev_t[1]));
    for (size_t k = 0; k + 1 < R; ++k) {
      if (bound(k + 2) == bound(k + 1)) continue;
      DeviceScope on(m->replicas[k].device);
      BLURRILY_HIP_TRY(hipEventElapsedTime(&ms, m->replicas[k].ev_t[0], m->replicas[k].ev_t[1]));
      worst = std::max(worst, ms);
    }
    m->last_find_ms = worst;
    m->last_tok_ms = 0.0;
  }
  return 0;
}

// ... and what a failure half-way must not leave behind: the timing mode switched off, replicas still searching and
// copying into the caller's buffers
int run_find_multi(trigram_map m, const char* d_packed, size_t packed_bytes, const uint64_t* d_offsets, size_t n,
                   uint16_t limit, trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb, hipStream_t stream) {
  const bool timing = m->timing;
  const int rc = run_find_multi_enqueue(m, d_packed, packed_bytes, d_offsets, n, limit, d_results, d_counts, d_nb, stream);
  if (rc < 0) {
    const int e = errno;
    m->timing = timing;
    for (Replica& r : m->replicas) {
      if (!r.stream) continue;
      DeviceScope on(r.device);
      (void)hipStreamSynchronize(r.stream);
    }
    (void)hipStreamSynchronize(stream);
    errno = e;
  }
  return rc;
}

// a batch goes over the replicas when "devices" asks for them and it is big enough to be worth a peer copy per
// device (and no request counters are being collected: they describe one launch sequence)
bool wants_multi(const trigram_map_t* m, size_t n) {
  return m->n_devices > 1 && !m->collect_stats && n >= size_t(1024) * m->n_devices;
}

}  // namespace detail
}  // namespace blurrily
