// refs.hip -- by reference: the extraction of references' trigrams from the device images (refs_extract) and the
// entry points blurrily_storage_get / _get_batch / _find_references[_device].
#include "map_internal.h"

using namespace blurrily;
using namespace blurrily::detail;

// ---- by reference (blurrily_storage_get / _get_batch / _find_references[_device]) ----------------------------------------
// The trigrams of n device-resident references, extracted on `stream` from the map as it is now: the base image minus its
// deleted ranks, the delta image of pending puts (kernels/refs.inc).  Each image uploads its reference table at its first
// such call.  *out describes the needles for run_find, and where the count of distinct references found and of the codes
// extracted for them sit on the device.
namespace blurrily {
namespace detail {

int refs_extract(trigram_map m, const uint32_t* d_refs, size_t n, hipStream_t stream, RefExtract* out) {
  if (n > kMaxBatchNeedles) { errno = EINVAL; return -1; }
  if (map_ready(m, stream) < 0) return -1;             // (every dirty bucket sorted: a find's needles would, as the device entry does)
  const bool with_delta = !log_of(m)->pending.empty() && m->delta.device >= 0;
  if (device_index_ensure_ref_table(&m->dev) < 0 || (with_delta && device_index_ensure_ref_table(&m->delta) < 0)) return -1;
  const uint32_t W = m->dev.n_windows + (with_delta ? m->delta.n_windows : 0u);
  const uint64_t max_tri = std::max<uint64_t>(1, std::max(m->dev.max_tri, with_delta ? m->delta.max_tri : 0u));
  const uint64_t entries = m->dev.n_entries + (with_delta ? m->delta.n_entries : 0u);
  const uint64_t code_slots = n + std::min<uint64_t>(uint64_t(n) * max_tri, entries);   // a pad of n, then every slot's codes
  constexpr size_t kWords = kWindowSize / 32;
  size_t at = 0;
  auto take = [&](size_t bytes) { const size_t here = at; at += align_up(std::max<size_t>(bytes, 8), 256); return here; };
  const size_t o_loc = take(n * sizeof(uint2)), o_req = take(size_t(W) * kWords * 4), o_wcnt = take(size_t(W) * 4);
  const size_t o_wbase = take((size_t(W) + 1) * 8), o_wpre = take(size_t(W) * kWords * 4), o_scnt = take(n * 4);
  const size_t o_sfill = take(n * 4), o_sstart = take((n + 1) * 8), o_codes = take(size_t(code_slots) * 2);
  const size_t o_ntri = take(n * 4), o_weight = take(n * 4), o_qoff = take(n * 8);
  if (m->ws_refs.reserve(at, stream) < 0) return -1;
  unsigned char* b = static_cast<unsigned char*>(m->ws_refs.p);
  RefArgs a{};
  auto image = [&](const DeviceIndex& ix, const uint32_t* tomb, uint32_t win0) {
    RefImage im{};
    im.sorted_ref = ix.d_sorted_ref; im.rank_of_pos = ix.d_rank_of_pos; im.n_refs = ix.n_refs; im.tomb = tomb;
    im.slice_se = ix.d_slice_se; im.ent = ix.d_ent; im.weight_of_rank = ix.d_weight_of_rank; im.dense_min8 = ix.dense_min8;
    im.win0 = win0;
    return im;
  };
  a.img[0] = image(m->dev, log_of(m)->n_tomb ? m->dev.d_tomb : nullptr, 0);
  a.n_img = 1;
  if (with_delta) { a.img[1] = image(m->delta, nullptr, m->dev.n_windows); a.n_img = 2; }
  a.n_win_all = W; a.refs = d_refs; a.n = uint32_t(n);
  a.loc = reinterpret_cast<uint2*>(b + o_loc); a.req = reinterpret_cast<uint32_t*>(b + o_req);
  a.win_cnt = reinterpret_cast<uint32_t*>(b + o_wcnt); a.win_base = reinterpret_cast<uint64_t*>(b + o_wbase);
  a.wprefix = reinterpret_cast<uint32_t*>(b + o_wpre); a.slot_cnt = reinterpret_cast<uint32_t*>(b + o_scnt);
  a.slot_fill = reinterpret_cast<uint32_t*>(b + o_sfill); a.slot_start = reinterpret_cast<uint64_t*>(b + o_sstart);
  a.codes = reinterpret_cast<uint16_t*>(b + o_codes); a.ntri = reinterpret_cast<uint32_t*>(b + o_ntri);
  a.weight = reinterpret_cast<uint32_t*>(b + o_weight); a.qoff = reinterpret_cast<uint64_t*>(b + o_qoff);
  if (launch_refs_extract(a, stream) < 0) return -1;
  out->needles = RefNeedles{a.codes, a.qoff, a.ntri, a.weight, uint32_t(n), code_slots};
  out->win_base_total = a.win_base + W;
  out->slot_start = a.slot_start;
  out->loc = a.loc;
  out->win0_delta = m->dev.n_windows;
  out->with_delta = with_delta;
  return 0;
}

int ExtractionOnHost::enqueue_counts(const RefExtract& from, hipStream_t stream) {
  x = from;
  BLURRILY_HIP_TRY(hipMemcpyAsync(ntri.data(), x.needles.ntri, n * 4, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(weight.data(), x.needles.weight, n * 4, hipMemcpyDeviceToHost, stream));
  return 0;
}

int ExtractionOnHost::read_offsets(hipStream_t stream) {
  uint64_t slots = 0;
  qoff = std::vector<uint64_t>(n);
  BLURRILY_HIP_TRY(hipMemcpyAsync(qoff.data(), x.needles.qoff, n * 8, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipMemcpyAsync(&slots, x.win_base_total, 8, hipMemcpyDeviceToHost, stream));
  BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  BLURRILY_HIP_TRY(hipMemcpy(&total, x.slot_start + slots, 8, hipMemcpyDeviceToHost));
  have_offsets = true;
  return 0;
}

int ExtractionOnHost::read_codes(hipStream_t stream) {
  if (have_codes) return 0;
  if (!have_offsets && read_offsets(stream) < 0) return -1;
  all = std::vector<uint16_t>(total);
  if (total) BLURRILY_HIP_TRY(hipMemcpy(all.data(), x.needles.codes + n, total * sizeof(uint16_t), hipMemcpyDeviceToHost));
  have_codes = true;
  return 0;
}

// The by-reference front end of the threshold and similarity finds: host references up and extracted.
int stage_reference_needles(trigram_map m, const uint32_t* references, size_t n, DeviceBuffer& buf, hipStream_t stream,
                            uint32_t* nb_trigrams, NeedleView* out) {
  if (buf.reserve(n * 4, stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(buf.p, references, n * 4, hipMemcpyHostToDevice, stream));
  RefExtract x;                                                // the by-reference front end (section 11)
  if (refs_extract(m, static_cast<const uint32_t*>(buf.p), n, stream, &x) < 0) return -1;
  if (nb_trigrams) {
    BLURRILY_HIP_TRY(hipMemcpyAsync(nb_trigrams, x.needles.ntri, n * 4, hipMemcpyDeviceToHost, stream));
    BLURRILY_HIP_TRY(hipStreamSynchronize(stream));
  }
  *out = NeedleView{x.needles.codes, x.needles.qoff, x.needles.ntri};
  return 0;
}

}  // namespace detail
}  // namespace blurrily

extern "C" {

int blurrily_storage_get_batch(trigram_map m, const uint32_t* references, size_t n, uint32_t* weights,
                               uint64_t* code_offsets, uint16_t* codes, size_t codes_cap) {
  if (!m || (n && (!references || !code_offsets))) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  if (n == 0) {
    if (ensure_device(m) < 0) return -1;                 // (no GPU: ENODEV, as for every other n)
    code_offsets[0] = 0;
    return 0;
  }
  hipStream_t stream = nullptr;
  // (the image first: without a GPU that is what fails, with ENODEV)
  if (m->host->dirty_buckets()) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  if (m->ws_io_in.reserve(n * sizeof(uint32_t), stream) < 0) return -1;
  BLURRILY_HIP_TRY(hipMemcpyAsync(m->ws_io_in.p, references, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  RefExtract x;
  if (refs_extract(m, static_cast<const uint32_t*>(m->ws_io_in.p), n, stream, &x) < 0) return -1;
  ExtractionOnHost R(n);
  if (R.enqueue_counts(x, stream) < 0 || R.read_offsets(stream) < 0) return -1;
  code_offsets[0] = 0;
  for (size_t i = 0; i < n; ++i) code_offsets[i + 1] = code_offsets[i] + R.ntri[i];
  if (weights)
    for (size_t i = 0; i < n; ++i) weights[i] = R.ntri[i] ? R.weight[i] : 0u;
  if (code_offsets[n] > codes_cap) { errno = ERANGE; return -1; }
  if (code_offsets[n] == 0) return 0;
  if (R.read_codes(stream) < 0) return -1;
  for (size_t i = 0; i < n; ++i)
    if (R.ntri[i]) std::memcpy(codes + code_offsets[i], R.codes_of(i), size_t(R.ntri[i]) * sizeof(uint16_t));
  return 0;
}

int blurrily_storage_get(trigram_map m, uint32_t reference, uint32_t* weight, int nb_trigrams, uint16_t* trigrams) {
  if (nb_trigrams < 0) { errno = EINVAL; return -1; }
  uint64_t off[2] = {0, 0};
  uint32_t w = 0;
  std::vector<uint16_t> codes(kNumCodes);                // (no reference holds more)
  if (blurrily_storage_get_batch(m, &reference, 1, &w, off, codes.data(), codes.size()) < 0) return -1;
  const int found = int(off[1]);
  if (found == 0) return 0;
  if (weight) *weight = w;
  if (trigrams) std::memcpy(trigrams, codes.data(), size_t(std::min(found, nb_trigrams)) * sizeof(uint16_t));
  return found;
}

int blurrily_storage_find_references_device(trigram_map m, const uint32_t* d_references, size_t n, uint16_t limit,
                                            trigram_match d_results, uint32_t* d_counts, uint32_t* d_nb_trigrams,
                                            void* stream) {
  DeviceScope scope(m->dev.device);
  hipStream_t st = static_cast<hipStream_t>(stream);
  if (n == 0) return ensure_device(m);
  RefExtract x;
  if (refs_extract(m, d_references, n, st, &x) < 0) return -1;
  // (the primary alone, whatever "devices" says; the rows do not depend on it)
  if (run_find(m, nullptr, 0, nullptr, n, limit, d_results, d_counts, nullptr, true, true, st, &x.needles) < 0) return -1;
  if (d_nb_trigrams)
    BLURRILY_HIP_TRY(hipMemcpyAsync(d_nb_trigrams, x.needles.ntri, n * sizeof(uint32_t), hipMemcpyDeviceToDevice, st));
  return 0;
}

int blurrily_storage_find_references(trigram_map m, const uint32_t* references, size_t n, uint16_t limit,
                                     trigram_match results, uint32_t* counts, uint32_t* nb_trigrams) {
  if (!m || (n && (!references || !counts || (limit && !results)))) { errno = EINVAL; return -1; }
  DeviceScope scope(m->dev.device);
  if (n == 0) return ensure_device(m);
  // (the image before the blocks, as in get_batch: without a GPU that is what fails, with ENODEV)
  if (m->host->dirty_buckets()) m->host->sort_dirty_buckets();
  if (ensure_device(m) < 0) return -1;
  hipStream_t stream = nullptr;
  const BatchBlocks B(n, 0, limit, true);               // (the references go in alone; out: [counts | nb_trigrams | rows])
  if (m->ws_io_in.reserve(n * sizeof(uint32_t), stream) < 0 || m->ws_io_out.reserve(B.out_bytes, stream) < 0) return -1;
  const BatchBlocks::Out out = B.out(static_cast<unsigned char*>(m->ws_io_out.p));
  BLURRILY_HIP_TRY(hipMemcpyAsync(m->ws_io_in.p, references, n * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  if (blurrily_storage_find_references_device(m, static_cast<const uint32_t*>(m->ws_io_in.p), n, limit, out.rows,
                                              out.counts, out.flags, stream) < 0)
    return -1;
  return B.copy_out(out.counts, out.flags, out.rows, counts, nb_trigrams, results, stream);
}

}  // extern "C"
