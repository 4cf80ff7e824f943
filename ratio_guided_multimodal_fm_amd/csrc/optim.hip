// optim.hip -- the optimizer step: global gradient norm, clip, Adam / AdamW and the weight EMA over a device-resident
// table of tensors (rgfm_adam_entry, include/rgfm.h), in two launches.
//
//   adam_norm_kernel  partials[b] = sum of g^2 over workgroup b's chunks, squares and sums in float64; one partial per
//                     workgroup, a fixed chunk -> workgroup assignment and fixed reduction trees: no atomics, the same
//                     bits on every run.
//   adam_step_kernel  every workgroup sums the ADAM_PARTIALS partials in the same order (so all hold the same norm),
//                     forms coef = min(1, max_norm / (norm + 1e-6)) and updates p, exp_avg, exp_avg_sq (and ema) of its
//                     chunks in one pass: 36 bytes per element with the EMA, 28 without.
//
// Work split.  The optimizer state is flat: tensor e owns floats [offset, offset + numel) of exp_avg / exp_avg_sq / ema,
// every offset a multiple of 4, the table sorted by offset.  A chunk is ADAM_CHUNK consecutive floats of that flat
// range, one quad of 4 per lane; since slots start on quads, a quad belongs to at most one tensor.  A chunk finds the
// entries it overlaps by binary search over the offsets; a chunk inside one tensor (nearly all of a real net's) needs
// nothing more, otherwise each lane searches that short range for its quad's tensor.  Quads in a slot's padding or in a
// hole of the table (a skipped parameter, another group's tensors) do nothing.  A workgroup owns a run of CONSECUTIVE
// chunks (a fixed assignment: chunk c belongs to workgroup c / chunks-per-workgroup), so after its first chunk the
// search is one load -- the next entry's offset, to see that the chunk is still inside the same tensor -- and the
// tensor's entry stays in registers.  (With a grid-stride assignment every chunk paid both binary searches, a chain of
// dependent table loads in front of its data loads: the norm kernel, which has little else to do, took 18.0 us instead
// of 12.8 us on the SVHN U-Net's 6.1 M elements; the step kernel's time is the same either way.)
//
// Alignment.  The state quad is always 16-byte aligned (the buffers are, rgfm_adam_step checks it).  The parameter and
// the gradient of a tensor are whatever the caller has: views into one gradient blob at any float offset.  A quad takes
// 16-byte loads and stores of p and g only when it is whole (not the tensor's tail) and that tensor's base pointer is
// 16-byte aligned; otherwise every element moves as a dword.  No unaligned 16-byte access is ever issued.
//
// Arithmetic.  Products and sums of the update run in float64 and are rounded to fp32 once per stored value; the
// square root and the quotient m / (sqrt(v) / sqrt(bc2) + eps) are fp32, as in torch.optim.Adam.
#include "rgfm_kernels.h"

namespace rgfm {

namespace {

constexpr int ADAM_THREADS = 256;
constexpr int ADAM_WAVES = ADAM_THREADS / 64;
static_assert(ADAM_CHUNK == ADAM_THREADS * 4, "one quad per lane and chunk");

// [lo, hi): the entries that can overlap floats [begin, end) -- lo the last entry starting at or before `begin` (0 if
// none), hi the first entry starting at or after `end`.  Uniform across the workgroup.
__device__ inline void chunk_entries(const rgfm_adam_entry* __restrict__ tab, int n, uint64_t begin, uint64_t end, int& lo,
                                     int& hi) {
  int a = 0, b = n;  // first entry with offset > begin
  while (a < b) {
    const int m = (a + b) >> 1;
    if (tab[m].offset <= begin) a = m + 1;
    else b = m;
  }
  lo = a > 0 ? a - 1 : 0;
  b = n;  // first entry with offset >= end (a is already a lower bound: offsets are increasing)
  if (a < n && tab[a].offset >= end) b = a;  // (the chunk ends inside entry lo, the usual case: one load, no second search)
  while (a < b) {
    const int m = (a + b) >> 1;
    if (tab[m].offset < end) a = m + 1;
    else b = m;
  }
  hi = a > lo ? a : lo + 1;
}

// The entry owning the quad at flat float `q`, or -1: the last entry of [lo, hi) starting at or before q, if q is inside it.
__device__ inline int quad_entry(const rgfm_adam_entry* __restrict__ tab, int lo, int hi, uint64_t q) {
  int a = lo, b = hi;  // first entry of the range with offset > q
  while (a < b) {
    const int m = (a + b) >> 1;
    if (tab[m].offset <= q) a = m + 1;
    else b = m;
  }
  if (a == lo) return -1;
  const int e = a - 1;
  return q - tab[e].offset < tab[e].numel ? e : -1;
}

// chunk_entries for the chunk after one whose range is [lo, hi), `begin` having grown: while the next entry starts at or
// behind `end` the chunk is still inside (or behind) entry lo -- one load; otherwise the full search.
__device__ inline void next_chunk_entries(const rgfm_adam_entry* __restrict__ tab, int n, uint64_t begin, uint64_t end,
                                          int& lo, int& hi) {
  if (lo + 1 >= n || tab[lo + 1].offset >= end) hi = lo + 1;
  else chunk_entries(tab, n, begin, end, lo, hi);
}

// The walk of one workgroup over its run of chunks: the entry range of the current chunk and a register copy of entry lo.
struct ChunkWalk {
  int lo = 0, hi = 0, cached = -1;
  rgfm_adam_entry ce;
  __device__ inline void move(const rgfm_adam_entry* __restrict__ tab, int n, uint64_t begin, bool first) {
    if (first) chunk_entries(tab, n, begin, begin + ADAM_CHUNK, lo, hi);
    else next_chunk_entries(tab, n, begin, begin + ADAM_CHUNK, lo, hi);
    if (cached != lo) ce = tab[lo], cached = lo;
  }
  // the entry owning the quad at flat float q into `t`; false: the quad belongs to no tensor of the table
  __device__ inline bool find(const rgfm_adam_entry* __restrict__ tab, uint64_t q, rgfm_adam_entry& t) const {
    if (hi == lo + 1) {  // one candidate: no table load
      t = ce;
      return q >= ce.offset && q - ce.offset < ce.numel;
    }
    const int e = quad_entry(tab, lo, hi, q);
    if (e < 0) return false;
    t = tab[e];
    return true;
  }
};

// the run of chunks [c0, c1) of this workgroup
__device__ inline void chunk_run(uint64_t n_chunks, uint64_t& c0, uint64_t& c1) {
  const uint64_t per = (n_chunks + gridDim.x - 1) / gridDim.x;
  c0 = blockIdx.x * per;
  c1 = c0 + per < n_chunks ? c0 + per : n_chunks;
}

__device__ inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

// Sum over the workgroup in a fixed order: lanes by xor-shuffle, then the waves' sums in wave order.  Every thread
// returns the total.
__device__ inline double block_sum(double v, double* lds) {
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  const int wave = threadIdx.x >> 6;
  __syncthreads();  // (lds may still be read from an earlier call)
  if ((threadIdx.x & 63) == 0) lds[wave] = v;
  __syncthreads();
  double t = 0.0;
  for (int w = 0; w < ADAM_WAVES; ++w) t += lds[w];
  return t;
}

}  // namespace

__global__ __launch_bounds__(ADAM_THREADS) void adam_norm_kernel(const rgfm_adam_entry* __restrict__ tab, int n,
                                                                 uint64_t span_begin, uint64_t n_chunks,
                                                                 double* __restrict__ partials) {
  __shared__ double lds[ADAM_WAVES];
  double acc = 0.0;
  uint64_t c0, c1;
  chunk_run(n_chunks, c0, c1);
  ChunkWalk w;
  for (uint64_t c = c0; c < c1; ++c) {
    const uint64_t begin = span_begin + c * ADAM_CHUNK;
    w.move(tab, n, begin, c == c0);
    const uint64_t q = begin + 4 * (uint64_t)threadIdx.x;
    rgfm_adam_entry t;
    if (!w.find(tab, q, t)) continue;
    const uint64_t i = q - t.offset;
    const uint64_t left = t.numel - i;
    const float* g = t.grad + i;
    if (left >= 4 && aligned16(t.grad)) {
      const float4 v = *reinterpret_cast<const float4*>(g);
      acc += (double)v.x * v.x;
      acc += (double)v.y * v.y;
      acc += (double)v.z * v.z;
      acc += (double)v.w * v.w;
    } else {
      const int k = left < 4 ? (int)left : 4;
      for (int j = 0; j < k; ++j) acc += (double)g[j] * g[j];
    }
  }
  const double total = block_sum(acc, lds);
  if (threadIdx.x == 0) partials[blockIdx.x] = total;
  // the slots no workgroup owns: zero, so that the step always sums ADAM_PARTIALS values
  if (blockIdx.x == 0)
    for (int b = gridDim.x + threadIdx.x; b < ADAM_PARTIALS; b += ADAM_THREADS) partials[b] = 0.0;
}

struct AdamElem {
  float p, m, v, ema;
};

template <bool EMA>
__device__ inline void adam_update(AdamElem& x, float g, const AdamStepArgs& a, double coef, double step_size, float sqrt_bc2) {
  double gd = coef * (double)g;
  double pd = (double)x.p;
  if (a.decoupled) pd *= a.decay_mul;          // p *= 1 - lr wd
  else if (a.wd != 0.0) gd += a.wd * pd;       // g += wd p
  x.m = (float)(a.beta1 * (double)x.m + a.one_minus_beta1 * gd);
  x.v = (float)(a.beta2 * (double)x.v + a.one_minus_beta2 * (gd * gd));
  const float denom = sqrtf(x.v) / sqrt_bc2 + a.eps;
  x.p = (float)(pd - step_size * (double)(x.m / denom));
  if (EMA) x.ema = (float)(a.ema_decay * (double)x.ema + a.one_minus_ema_decay * (double)x.p);
}

template <bool EMA>
__global__ __launch_bounds__(ADAM_THREADS) void adam_step_kernel(AdamStepArgs a) {
  __shared__ double lds[ADAM_WAVES];
  double coef = 1.0;
  if (a.partials) {
    double s = 0.0;
    for (int b = threadIdx.x; b < ADAM_PARTIALS; b += ADAM_THREADS) s += a.partials[b];
    const double norm = sqrt(block_sum(s, lds));
    if (a.max_norm > 0.0) coef = fmin(1.0, a.max_norm / (norm + 1e-6));
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.grad_norm_out) *a.grad_norm_out = (float)norm;
  }
  const rgfm_adam_entry* __restrict__ tab = a.tab;
  uint64_t c0, c1;
  chunk_run(a.n_chunks, c0, c1);
  ChunkWalk w;
  for (uint64_t c = c0; c < c1; ++c) {
    const uint64_t begin = a.span_begin + c * ADAM_CHUNK;
    w.move(tab, a.n, begin, c == c0);
    const uint64_t q = begin + 4 * (uint64_t)threadIdx.x;
    rgfm_adam_entry t;
    if (!w.find(tab, q, t)) continue;
    const uint64_t i = q - t.offset;
    const uint64_t left = t.numel - i;
    const double step_size = a.lr / t.bc1;
    const float sqrt_bc2 = (float)sqrt(t.bc2);
    float* p = t.param + i;
    const float* g = t.grad + i;
    // the state quad: 16-byte aligned whatever the tensor (slots are padded to whole quads)
    float4 m4 = *reinterpret_cast<const float4*>(a.exp_avg + q);
    float4 v4 = *reinterpret_cast<const float4*>(a.exp_avg_sq + q);
    float4 e4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (EMA) e4 = *reinterpret_cast<const float4*>(a.ema + q);
    const int k = left < 4 ? (int)left : 4;
    const bool vec = k == 4 && aligned16(t.param) && aligned16(t.grad);
    float pv[4] = {0.f, 0.f, 0.f, 0.f}, gv[4] = {0.f, 0.f, 0.f, 0.f};
    if (vec) {
      const float4 p4 = *reinterpret_cast<const float4*>(p);
      const float4 g4 = *reinterpret_cast<const float4*>(g);
      pv[0] = p4.x, pv[1] = p4.y, pv[2] = p4.z, pv[3] = p4.w;
      gv[0] = g4.x, gv[1] = g4.y, gv[2] = g4.z, gv[3] = g4.w;
    } else {
      for (int j = 0; j < 4; ++j)
        if (j < k) pv[j] = p[j], gv[j] = g[j];
    }
    float mv[4] = {m4.x, m4.y, m4.z, m4.w}, vv[4] = {v4.x, v4.y, v4.z, v4.w}, ev[4] = {e4.x, e4.y, e4.z, e4.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < k) {  // (the padding of a slot keeps its zeros)
        AdamElem x{pv[j], mv[j], vv[j], ev[j]};
        adam_update<EMA>(x, gv[j], a, coef, step_size, sqrt_bc2);
        pv[j] = x.p, mv[j] = x.m, vv[j] = x.v, ev[j] = x.ema;
      }
    }
    if (vec) {
      *reinterpret_cast<float4*>(p) = make_float4(pv[0], pv[1], pv[2], pv[3]);
    } else {
      for (int j = 0; j < 4; ++j)
        if (j < k) p[j] = pv[j];
    }
    *reinterpret_cast<float4*>(a.exp_avg + q) = make_float4(mv[0], mv[1], mv[2], mv[3]);
    *reinterpret_cast<float4*>(a.exp_avg_sq + q) = make_float4(vv[0], vv[1], vv[2], vv[3]);
    if (EMA) *reinterpret_cast<float4*>(a.ema + q) = make_float4(ev[0], ev[1], ev[2], ev[3]);
  }
}

static unsigned adam_grid(uint64_t n_chunks, unsigned cap) { return (unsigned)(n_chunks < cap ? n_chunks : cap); }

void launch_adam_norm(const rgfm_adam_entry* tab, int n, uint64_t span_begin, uint64_t span_end, double* partials,
                      hipStream_t s) {
  const uint64_t n_chunks = (span_end - span_begin + ADAM_CHUNK - 1) / ADAM_CHUNK;
  hipLaunchKernelGGL(adam_norm_kernel, dim3(adam_grid(n_chunks, ADAM_PARTIALS)), dim3(ADAM_THREADS), 0, s, tab, n, span_begin,
                     n_chunks, partials);
}

void launch_adam_step(AdamStepArgs a, uint64_t span_end, hipStream_t s) {
  a.n_chunks = (span_end - a.span_begin + ADAM_CHUNK - 1) / ADAM_CHUNK;
  const dim3 grid(adam_grid(a.n_chunks, ADAM_MAX_GRID)), block(ADAM_THREADS);
  if (a.ema) hipLaunchKernelGGL(adam_step_kernel<true>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(adam_step_kernel<false>, grid, block, 0, s, a);
}

}  // namespace rgfm
