// kernels/refs.inc -- by reference: a reference's trigrams read back out of the device image, and the needle arrays of
// the find path filled from them (blurrily_storage_get / _get_batch / _find_references, DESIGN.md section 11).
// Part of find_kernels.hip (timed build only: included in namespace blurrily, in front of the launch functions).
//
// A reference lives in one window of one image (base or delta) as its in-window rank r; its trigrams are the codes c whose
// (window, c) slice holds r.  The extraction visits every slice of every TOUCHED window once, whatever the number of ranks
// requested there:
//   refs_lookup_kernel   reference -> (image, rank) by a binary search of the image's sorted references (deleted base ranks
//                        are passed over); marks the rank in its window's request bitmap (kWindowSize bits) and counts the
//                        window's distinct requests.  A scan over the windows numbers the requested ranks: slots.
//   refs_slices_kernel   grid (window, chunk of kRefCodes codes): the window's request bitmap in LDS, one lane per code of
//                        the chunk -- its slice bounds, a short sparse slice's postings (16-byte loads) tested against the
//                        bitmap; long sparse slices and dense slices (their inline bitmap ANDed with the requests, only at
//                        the words that hold a request) go to the waves, one slice per wave.  Pass 0 counts a slot's codes,
//                        pass 1 (after a scan) writes them.
//   refs_sort_kernel     a slot's codes ascending (they arrive in no order: chunks and lanes race).
//   refs_emit_kernel     per reference: trigram count, weight, where its codes start.
//   ref_needles_kernel   what tokenise_kernel leaves for the find kernels, per image run: q_ntri, q_nb (the image's bucket
//                        sizes), q_start (start_win[weight]), the mid / big lists.

namespace {

constexpr uint32_t kRefThreads = 256;   // refs_slices_kernel: one lane per code of its chunk
constexpr uint32_t kRefCodes   = kRefThreads;
constexpr uint32_t kRefWords   = kWindowSize / 32;   // request bitmap words per window
constexpr uint32_t kRefLaneMax = 64;    // sparse slices of up to this many entries are tested by their code's lane alone

__global__ void refs_lookup_kernel(const RefArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint32_t ref = A.refs[i];
  uint2 loc = make_uint2(0xFFFFFFFFu, 0u);
  for (uint32_t k = 0; k < A.n_img; ++k) {
    const RefImage& im = A.img[k];
    uint32_t lo = 0, hi = im.n_refs;                    // first position with sorted_ref >= ref
    while (lo < hi) {
      const uint32_t mid = (lo + hi) >> 1;
      if (im.sorted_ref[mid] < ref) lo = mid + 1; else hi = mid;
    }
    if (lo >= im.n_refs || im.sorted_ref[lo] != ref) continue;
    const uint32_t rank = im.rank_of_pos[lo];
    if (im.tomb && ((im.tomb[rank >> 5] >> (rank & 31u)) & 1u)) continue;    // deleted since the build (maybe put again: delta)
    const uint32_t wa = im.win0 + rank / kWindowRanks, r = rank % kWindowRanks;
    const uint32_t bit = 1u << (r & 31u);
    const uint32_t old = atomicOr(&A.req[size_t(wa) * kRefWords + (r >> 5)], bit);
    if (!(old & bit)) atomicAdd(&A.win_cnt[wa], 1u);
    loc = make_uint2(wa, r);
    break;
  }
  A.loc[i] = loc;
}

// Exclusive prefix sum of in[0, m) into out[0, m] (out[m]: the total) by one workgroup; m = *m_dev when m_dev is set.
__global__ __launch_bounds__(1024) void refs_scan_kernel(const uint32_t* __restrict__ in, uint64_t* __restrict__ out,
                                                         uint32_t m, const uint64_t* __restrict__ m_dev) {
  __shared__ uint64_t s_sum[1024];
  if (m_dev) m = uint32_t(*m_dev);
  const uint32_t t = threadIdx.x, per = (m + 1023u) / 1024u;
  const uint32_t a = min(m, t * per), b = min(m, a + per);
  uint64_t sum = 0;
  for (uint32_t k = a; k < b; ++k) sum += in[k];
  s_sum[t] = sum;
  __syncthreads();
  for (uint32_t d = 1; d < 1024; d <<= 1) {             // inclusive scan over the threads' sums
    const uint64_t v = t >= d ? s_sum[t - d] : 0ull;
    __syncthreads();
    s_sum[t] += v;
    __syncthreads();
  }
  uint64_t run = s_sum[t] - sum;
  for (uint32_t k = a; k < b; ++k) { out[k] = run; run += in[k]; }
  if (t == 1023) out[m] = s_sum[1023];
}

// The slot of in-window rank r (its bit set in s_req): the window's first slot + the requests in front of it.
__device__ __forceinline__ uint32_t refs_slot(const uint32_t* s_req, const uint32_t* s_pre, uint32_t base, uint32_t r) {
  return base + s_pre[r >> 5] + __popc(s_req[r >> 5] & ((1u << (r & 31u)) - 1u));
}

template <bool WRITE>
__device__ __forceinline__ void refs_hit(const RefArgs& A, uint32_t slot, uint16_t code) {
  if (WRITE) {
    const uint32_t at = atomicAdd(&A.slot_fill[slot], 1u);
    A.codes[A.n + A.slot_start[slot] + at] = code;
  } else {
    atomicAdd(&A.slot_cnt[slot], 1u);
  }
}

template <bool WRITE>
__global__ __launch_bounds__(kRefThreads) void refs_slices_kernel(const RefArgs A) {
  const uint32_t wa = blockIdx.x, tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
  if (A.win_cnt[wa] == 0) return;                       // no reference of this window requested
  const uint32_t k = (A.n_img > 1 && wa >= A.img[1].win0) ? 1u : 0u;
  const RefImage& im = A.img[k];
  const uint32_t w = wa - im.win0;
  __shared__ uint32_t s_req[kRefWords], s_pre[kRefWords], s_nz[kRefWords];
  __shared__ uint32_t s_long[kRefCodes];
  __shared__ uint32_t s_part[kRefThreads], s_n_nz, s_n_long;
  // the window's requests, the requests in front of every word, the words that hold any
  constexpr uint32_t kPer = kRefWords / kRefThreads;
  uint32_t cnt = 0;
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint32_t v = A.req[size_t(wa) * kRefWords + tid * kPer + j];
    s_req[tid * kPer + j] = v;
    cnt += __popc(v);
  }
  s_part[tid] = cnt;
  if (tid == 0) { s_n_nz = 0; s_n_long = 0; }
  __syncthreads();
  for (uint32_t d = 1; d < kRefThreads; d <<= 1) {
    const uint32_t v = tid >= d ? s_part[tid - d] : 0u;
    __syncthreads();
    s_part[tid] += v;
    __syncthreads();
  }
  uint32_t run = s_part[tid] - cnt;
  for (uint32_t j = 0; j < kPer; ++j) {
    const uint32_t at = tid * kPer + j, v = s_req[at];
    s_pre[at] = run;
    run += __popc(v);
    if (v) s_nz[atomicAdd(&s_n_nz, 1u)] = at;
  }
  __syncthreads();
  if (!WRITE && blockIdx.y == 0)                        // (refs_emit_kernel finds a reference's slot through these)
    for (uint32_t j = tid; j < kRefWords; j += kRefThreads) A.wprefix[size_t(wa) * kRefWords + j] = s_pre[j];
  const uint32_t base = uint32_t(A.win_base[wa]), n_nz = s_n_nz;
  const uint32_t dense_min8 = im.dense_min8;
  // one lane per code: short sparse slices here, the rest listed for the waves
  const uint32_t code = blockIdx.y * kRefCodes + tid;
  if (code < kNumCodes) {
    const uint2 se = im.slice_se[size_t(w) * kNumCodes + code];
    const uint32_t len = se.y - se.x;
    if (len > kRefLaneMax || (len != 0 && len >= dense_min8)) {
      s_long[atomicAdd(&s_n_long, 1u)] = code;
    } else {
      const uint4* p = reinterpret_cast<const uint4*>(im.ent + se.x);   // (slices start on 16 bytes, padded to 8 entries)
      for (uint32_t g = 0; g < len / 8u; ++g) {
        const uint4 v = p[g];
        const uint32_t h[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t r = (h[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
          if (r != kPadRank && ((s_req[r >> 5] >> (r & 31u)) & 1u))
            refs_hit<WRITE>(A, refs_slot(s_req, s_pre, base, r), uint16_t(code));
        }
      }
    }
  }
  __syncthreads();
  // one slice per wave: long sparse slices streamed (512 postings a wave-load), dense ones asked at the requested words
  const uint32_t n_long = s_n_long;
  for (uint32_t s = wave; s < n_long; s += kRefThreads / 64u) {
    const uint32_t c = s_long[s];
    const uint2 se = im.slice_se[size_t(w) * kNumCodes + c];
    const uint32_t len = se.y - se.x;
    if (len >= dense_min8) {
      const uint32_t* bm = reinterpret_cast<const uint32_t*>(im.ent + (se.x - kBitmapSlots));
      for (uint32_t z = lane; z < n_nz; z += 64u) {
        const uint32_t j = s_nz[z];
        uint32_t hit = bm[j] & s_req[j];
        while (hit) {
          const uint32_t b = __ffs(hit) - 1u;
          hit &= hit - 1u;
          refs_hit<WRITE>(A, base + s_pre[j] + __popc(s_req[j] & ((1u << b) - 1u)), uint16_t(c));
        }
      }
    } else {
      const uint4* p = reinterpret_cast<const uint4*>(im.ent + se.x);
      for (uint32_t g = lane; g < len / 8u; g += 64u) {
        const uint4 v = p[g];
        const uint32_t h[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e) {
          const uint32_t r = (h[e >> 1] >> ((e & 1) * 16)) & 0xFFFFu;
          if (r != kPadRank && ((s_req[r >> 5] >> (r & 31u)) & 1u))
            refs_hit<WRITE>(A, refs_slot(s_req, s_pre, base, r), uint16_t(c));
        }
      }
    }
  }
}

// a slot's codes ascending: up to 64 in the lane's LDS row, longer ones by a heap sort in place
__global__ __launch_bounds__(128) void refs_sort_kernel(const RefArgs A) {
  __shared__ uint16_t s_row[128][66];
  const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
  if (s >= uint32_t(A.win_base[A.n_win_all])) return;
  const uint32_t m = A.slot_cnt[s];
  uint16_t* out = A.codes + A.n + A.slot_start[s];
  if (m <= 64) {
    uint16_t* row = s_row[threadIdx.x];
    for (uint32_t k = 0; k < m; ++k) row[k] = out[k];
    for (uint32_t i = 1; i < m; ++i) {
      const uint16_t v = row[i];
      uint32_t j = i;
      while (j > 0 && row[j - 1] > v) { row[j] = row[j - 1]; --j; }
      row[j] = v;
    }
    for (uint32_t k = 0; k < m; ++k) out[k] = row[k];
    return;
  }
  auto sift = [&](uint32_t root, uint32_t lim) {
    for (;;) {
      uint32_t child = 2 * root + 1;
      if (child >= lim) return;
      if (child + 1 < lim && out[child] < out[child + 1]) ++child;
      if (out[root] >= out[child]) return;
      const uint16_t t = out[root]; out[root] = out[child]; out[child] = t;
      root = child;
    }
  };
  for (uint32_t i = m / 2; i-- > 0;) sift(i, m);
  for (uint32_t lim = m; lim-- > 1;) {
    const uint16_t t = out[0]; out[0] = out[lim]; out[lim] = t;
    sift(0, lim);
  }
}

// per reference: its trigram count (0: not in the map), its weight, and qoff[i] with its codes at codes + qoff[i] + i --
// the find kernels' "needle q's codes at qcodes + offsets[q] + q".  codes[0, n) is a pad: qoff never underflows.
__global__ void refs_emit_kernel(const RefArgs A) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= A.n) return;
  const uint2 loc = A.loc[i];
  uint32_t ntri = 0, weight = 0;
  uint64_t at = A.n;
  if (loc.x != 0xFFFFFFFFu) {
    const uint32_t wa = loc.x, r = loc.y;
    const uint32_t word = A.req[size_t(wa) * kRefWords + (r >> 5)];
    const uint32_t slot = uint32_t(A.win_base[wa]) + A.wprefix[size_t(wa) * kRefWords + (r >> 5)] +
                          __popc(word & ((1u << (r & 31u)) - 1u));
    const uint32_t k = (A.n_img > 1 && wa >= A.img[1].win0) ? 1u : 0u;
    ntri = A.slot_cnt[slot];
    weight = A.img[k].weight_of_rank[(wa - A.img[k].win0) * kWindowRanks + r];
    at = A.n + A.slot_start[slot];
  }
  A.ntri[i] = ntri;
  A.weight[i] = weight;
  A.qoff[i] = at - i;
}

__global__ void ref_needles_kernel(const RefNeedles R, const uint32_t* __restrict__ code_total,
                                   const uint32_t* __restrict__ start_win, uint32_t* __restrict__ q_ntri,
                                   uint32_t* __restrict__ q_nb, uint32_t* __restrict__ q_start,
                                   uint32_t* __restrict__ big_list, uint32_t* __restrict__ big_count,
                                   uint32_t* __restrict__ mid_list, uint32_t* __restrict__ mid_count) {
  const uint32_t q = blockIdx.x * blockDim.x + threadIdx.x;
  if (q >= R.n) return;
  const uint32_t d = R.ntri[q];
  const uint16_t* codes = R.codes + (R.qoff[q] + q);
  uint64_t nb = 0;
  for (uint32_t k = 0; k < d; ++k) nb += code_total[codes[k]];
  q_ntri[q] = d;
  // a reference has no length: its weight stands in (its string's length when it was put with weight 0)
  const uint32_t wgt = R.weight[q];
  q_start[q] = start_win[wgt < 255u ? wgt : 255u];
  q_nb[q] = nb > 0xFFFFFFFFull ? 0xFFFFFFFFu : uint32_t(nb);
  if (d > 127) big_list[atomicAdd(big_count, 1u)] = q;
  else if (d > 64) mid_list[atomicAdd(mid_count, 1u)] = q;
}

}  // namespace

// ------------------------------------------------------------------ launch ---

int launch_refs_extract(const RefArgs& a, hipStream_t stream) {
  if (a.n == 0) return 0;
  const uint32_t W = a.n_win_all;
  BLURRILY_HIP_TRY(hipMemsetAsync(a.req, 0, size_t(W) * kRefWords * sizeof(uint32_t), stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(a.win_cnt, 0, size_t(W) * sizeof(uint32_t), stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(a.slot_cnt, 0, size_t(a.n) * sizeof(uint32_t), stream));
  BLURRILY_HIP_TRY(hipMemsetAsync(a.slot_fill, 0, size_t(a.n) * sizeof(uint32_t), stream));
  const dim3 per_ref((a.n + 255) / 256), chunks(W, (kNumCodes + kRefCodes - 1) / kRefCodes);
  hipLaunchKernelGGL(refs_lookup_kernel, per_ref, dim3(256), 0, stream, a);
  hipLaunchKernelGGL(refs_scan_kernel, dim3(1), dim3(1024), 0, stream, a.win_cnt, a.win_base, W, nullptr);
  hipLaunchKernelGGL(refs_slices_kernel<false>, chunks, dim3(kRefThreads), 0, stream, a);
  hipLaunchKernelGGL(refs_scan_kernel, dim3(1), dim3(1024), 0, stream, a.slot_cnt, a.slot_start, 0u, a.win_base + W);
  hipLaunchKernelGGL(refs_slices_kernel<true>, chunks, dim3(kRefThreads), 0, stream, a);
  hipLaunchKernelGGL(refs_sort_kernel, dim3((a.n + 127) / 128), dim3(128), 0, stream, a);
  hipLaunchKernelGGL(refs_emit_kernel, per_ref, dim3(256), 0, stream, a);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}

int launch_ref_needles(const RefNeedles& r, const uint32_t* code_total, const uint32_t* start_win, uint32_t* q_ntri,
                       uint32_t* q_nb, uint32_t* q_start, uint32_t* big_list, uint32_t* big_count, uint32_t* mid_list,
                       uint32_t* mid_count, hipStream_t stream) {
  if (r.n == 0) return 0;
  note_launch("ref_needles_kernel");
  hipLaunchKernelGGL(ref_needles_kernel, dim3((r.n + 127) / 128), dim3(128), 0, stream, r, code_total, start_win, q_ntri,
                     q_nb, q_start, big_list, big_count, mid_list, mid_count);
  BLURRILY_HIP_TRY(hipGetLastError());
  return 0;
}
