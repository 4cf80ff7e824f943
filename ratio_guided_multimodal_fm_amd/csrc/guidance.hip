// guidance.hip -- MC importance-weighted guidance (mc_feng) and the Euler update.
//
// Replaces the per-step guidance block of the reference samplers
// (src/sample_mnist_svhn.py:124-171, src/utils/flow_utils.py:273-369), which
// materialises six [B, N, D] broadcast temporaries per step, by two passes that
// never leave registers/LDS:
//   guid_logp : l[b,i] = -0.5 (|x_b - t m^x_i|^2 / s2) + -0.5 (|y_b - t m^y_i|^2 / s2)
//               (direct differences, no GEMM expansion: late-time weights are
//               scaled by 1/sigma_t^2 ~ 8e3 and cancellation would flip near-ties)
//   guid_apply: row-normalised importance weights (exact reference epsilon
//               sequence), g = sum_i w_i (m_i - x)/(1 - t + eps) as an fp32-MFMA
//               GEMM [B,N] x [N,D], blend (1-gamma) v + gamma g, and optionally the
//               Euler update.
//   guid_cross_*: with cross pairing (all N x N pairs of the MC set) the weights stage between the two: one marginal
//               weight row per modality from the distance slices and the ratio matrix (below, "cross pairing")
// guid_logp is a VALU-bound elementwise reduction, guid_apply a small fp32 GEMM; the MC set
// (N x D) stays L2-resident.
#include "rgfm_device.h"

namespace rgfm {

constexpr int GD = 64;        // D-chunk
constexpr int GLD = GD + 4;   // LDS row stride (floats): conflict-free b128 rows

// Squared distances, sliced along D: block (bx, by, z) adds up slice z of one modality for a 32 x 64 tile of
// (row, MC sample) pairs and writes the fp64 partial sum; guid_apply adds the slices (fp64 sums of fp32 chunk
// partials are exact, so the slicing does not change a bit) -- 4x the workgroups of an unsliced launch at the
// benchmark shape, where 16 x 8 tiles would leave half of the 256 CUs idle on a kernel that nothing overlaps.
// the step's scalars: launch arguments, or (hipGraph replay) the schedule row of the device-side step counter
__device__ __forceinline__ GuidanceArgs with_schedule(const GuidanceArgs& in) {
  GuidanceArgs a = in;
  if (in.sched) {
    const float* q = in.sched + 4 * (size_t)*in.step_ptr;
    a.tf = q[0], a.s2 = q[1], a.cden = q[2];
  }
  return a;
}

// Thread = 2 rows x 4 MC samples of a 32 x 64 tile; the differences and squares are packed-fp32 instructions (two
// elements each: v_pk_add_f32, v_pk_fma_f32 -- full rate where no MFMA runs beside them), accumulated per element parity and
// added at the end of a 64-element chunk.  The next chunk's rows are fetched into registers while this one is multiplied.
typedef float f32x2 __attribute__((ext_vector_type(2)));
// a - b on both halves in one instruction (hipcc scalarises a v2f32 subtraction, also when written as a + (-b) or fma(b, -1, a))
__device__ __forceinline__ f32x2 pk_sub(f32x2 a, f32x2 b) {
  f32x2 d;
  asm("v_pk_add_f32 %0, %1, %2 neg_lo:[0,1] neg_hi:[0,1]" : "=v"(d) : "v"(a), "v"(b));
  return d;
}
__global__ __launch_bounds__(256) void guid_logp_kernel(const GuidanceArgs a_in) {
  const GuidanceArgs a = with_schedule(a_in);
  __shared__ __attribute__((aligned(16))) float sx[32 * GLD];
  __shared__ __attribute__((aligned(16))) float sm[64 * GLD];
  const int tid = threadIdx.x;
  const int tb = tid >> 4, ti = tid & 15;
  const int bb = blockIdx.x * 32, ib = blockIdx.y * 64;
  const int z = blockIdx.z;
  const int part = z >= a.nsx ? 1 : 0;
  const float* X = part ? a.y : a.x;
  const float* M = part ? a.mc_y1 : a.mc_x1;
  const int D = part ? a.dy : a.dx;
  const int dbeg = (part ? z - a.nsx : z) * a.slice_len;
  const int dend = dbeg + a.slice_len < D ? dbeg + a.slice_len : D;
  // staging items: item it < 512 is (row it / 16, float4 it % 16) of x, the 1024 behind them of the MC set; six per thread
  const float* src[6];
  bool ok[6];
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    const int it = tid + 256 * j;
    const bool isx = it < 512;
    const int row = isx ? it >> 4 : (it - 512) >> 4;
    const int grow = isx ? bb + row : ib + row;
    ok[j] = isx ? grow < a.B : grow < a.N;
    src[j] = (isx ? X : M) + (size_t)(ok[j] ? grow : 0) * D;  // (the row; the float4 inside it: fetch)
  }
  f32x4 rv[6];
  auto fetch = [&](int d0) {
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int d = d0 + (tid & 15) * 4;
      const bool in = ok[j] && d < dend;
      const f32x4 v = *reinterpret_cast<const f32x4*>(src[j] + (in ? d : 0));  // (clamped to the row's first float4: always valid)
      rv[j] = in ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    }
  };
  // chunk partials in fp32 (64 terms), running total in fp64: the sum is then exact
  // to fp32 rounding, which matters because l is later scaled by 1/sigma_t^2 (up to ~8e3)
  double S[2][4];
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) S[p][q] = 0.0;
  fetch(dbeg);
  for (int d0 = dbeg; d0 < dend; d0 += GD) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const int it = tid + 256 * j;
      f32x4 v = rv[j];
      if (it >= 512) {  // mu = t * x_1 (rounded, as the reference)
        v.x = __fmul_rn(a.tf, v.x), v.y = __fmul_rn(a.tf, v.y), v.z = __fmul_rn(a.tf, v.z), v.w = __fmul_rn(a.tf, v.w);
        *reinterpret_cast<f32x4*>(sm + ((it - 512) >> 4) * GLD + (it & 15) * 4) = v;
      } else {
        *reinterpret_cast<f32x4*>(sx + (it >> 4) * GLD + (it & 15) * 4) = v;
      }
    }
    __syncthreads();
    if (d0 + GD < dend) fetch(d0 + GD);
    f32x2 c[2][4];
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) c[p][q] = f32x2{0.f, 0.f};
#pragma unroll
    for (int d = 0; d < GD; d += 4) {
      f32x4 xv[2], mv[4];
#pragma unroll
      for (int p = 0; p < 2; ++p) xv[p] = *reinterpret_cast<const f32x4*>(sx + (tb + 16 * p) * GLD + d);
#pragma unroll
      for (int q = 0; q < 4; ++q) mv[q] = *reinterpret_cast<const f32x4*>(sm + (ti + 16 * q) * GLD + d);
#pragma unroll
      for (int p = 0; p < 2; ++p)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const f32x2 d0v = pk_sub(f32x2{xv[p].x, xv[p].y}, f32x2{mv[q].x, mv[q].y});
          const f32x2 d1v = pk_sub(f32x2{xv[p].z, xv[p].w}, f32x2{mv[q].z, mv[q].w});
          c[p][q] = __builtin_elementwise_fma(d0v, d0v, c[p][q]);
          c[p][q] = __builtin_elementwise_fma(d1v, d1v, c[p][q]);
        }
    }
#pragma unroll
    for (int p = 0; p < 2; ++p)
#pragma unroll
      for (int q = 0; q < 4; ++q) S[p][q] += (double)(c[p][q].x + c[p][q].y);
  }
#pragma unroll
  for (int p = 0; p < 2; ++p)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int b = bb + tb + 16 * p, i = ib + ti + 16 * q;
      if (b < a.B && i < a.N) a.dist[((size_t)z * a.B + b) * a.N + i] = S[p][q];
    }
}

// l[b,i] = -0.5 |x_b - t m^x_i|^2 / s2 + -0.5 |y_b - t m^y_i|^2 / s2 from the sliced sums (each modality's
// term rounded to fp32 on its own, then added: the reference's two-statement form, :141-143)
__device__ __forceinline__ float logp_of(const GuidanceArgs& a, int b, int i) {
  double sx = 0.0, sy = 0.0;
  for (int z = 0; z < a.nsx; ++z) sx += a.dist[((size_t)z * a.B + b) * a.N + i];
  for (int z = a.nsx; z < a.nsx + a.nsy; ++z) sy += a.dist[((size_t)z * a.B + b) * a.N + i];
  const float lx = __fadd_rn(0.f, __fmul_rn(-0.5f, (float)sx) / a.s2);
  return __fadd_rn(lx, __fmul_rn(-0.5f, (float)sy) / a.s2);
}

__device__ __forceinline__ float wave_sum_g(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
  return v;
}
__device__ __forceinline__ float wave_max_g(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
  return v;
}

// Importance weights of one row per wave (sample_mnist_svhn.py:146-156), written once per step to a.wbuf [B][N]
// (and to weights_out when the caller asks for them): guid_apply's workgroups -- sixteen column blocks per row
// block -- read them back instead of each recomputing the softmax from the distance slices.
__global__ __launch_bounds__(256) void guid_weights_kernel(const GuidanceArgs a_in) {
  const GuidanceArgs a = with_schedule(a_in);
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [4][N]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const int b = blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  float* swr = sw + (size_t)wave * N;
  const float* ratios = a.mc_ratios + (size_t)b * a.ratio_stride;  // (the shared vector, or this row's own)
  float mx = -INFINITY;
  for (int i = lane; i < N; i += 64) {
    const float l = logp_of(a, b, i);
    swr[i] = l;
    mx = fmaxf(mx, l);
  }
  mx = wave_max_g(mx);
  float ps = 0.f, zs = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float p = expf(swr[i] - mx);
    swr[i] = p;
    ps += p;
    zs += __fmul_rn(ratios[i], p);
  }
  ps = wave_sum_g(ps);
  zs = wave_sum_g(zs);
  const float pbar = __fadd_rn(ps / (float)N, 1e-10f);
  const float zbar = __fadd_rn(zs / (float)N, 1e-10f);
  if (a.diag_rec && lane == 0) a.diag_rec[(size_t)b * RGFM_DIAG_FLOATS + RGFM_DIAG_Z_BAR] = zbar;
  float ws = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float w = __fmul_rn(ratios[i] / zbar, swr[i] / pbar);
    swr[i] = w;
    ws += w;
  }
  ws = __fadd_rn(wave_sum_g(ws), 1e-10f);
  float rsum = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float w = swr[i] / ws;
    a.wbuf[(size_t)b * N + i] = w;
    if (a.weights_out) a.weights_out[(size_t)b * N + i] = w;
    rsum += w;
  }
  rsum = wave_sum_g(rsum);  // the row's weight sum as guid_apply_mfma_kernel needs it (1 up to rounding and the epsilon)
  if (lane == 0) a.wsum[b] = rsum;
}

// The same weights, held to an effective-sample-size floor (include/rgfm.h, "Effective-sample-size floor").  The first
// half is guid_weights_kernel statement by statement -- the row's weights w of today, its Z_bar, its sum -- with the
// log-density terms kept beside them (LDS: sl [4][N] and sw [4][N]).  ESS_1 = (sum w)^2 / sum w^2 in
// guid_diag_wstats_kernel's arithmetic, n_pos = #{r_i > 0}, E* = min(ess_min, n_pos).  A row with ESS_1 >= E* (or E* <= 1,
// or no positive ratio) leaves as guid_weights_kernel writes it, tau = 1: the tempered formula is never evaluated there.
// A collapsed row: d_i = L_i - max_P L, L_i = l_i + log r_i over P = {r_i > 0} (samples outside P carry the marker -inf
// and enter every sum as an exact 0: tau * -inf is never formed), 40 bisection steps on tau in [0, 1] for
// ESS(tau) = (sum e^{tau d})^2 / sum e^{2 tau d} >= E* (one expf per sample and step, no early exit, no epsilon: the
// largest term is 1), tau = lo, w_i = e^{tau d_i} / sum.  Every sum: lane l over samples l, l + 64, ... in index order,
// then the xor butterfly -- fixed by N, so a row's result is the same in every batch.  Each lane reads back only the LDS
// entries it wrote itself: no barrier.
constexpr int ESS_BISECT = 40;
__global__ __launch_bounds__(256) void guid_weights_ess_kernel(const GuidanceArgs a_in) {
  const GuidanceArgs a = with_schedule(a_in);
  extern __shared__ __attribute__((aligned(16))) float sw[];  // [4][N] weights, then [4][N] log-weights
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int N = a.N;
  const int b = blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  float* swr = sw + (size_t)wave * N;
  float* slr = sw + (size_t)(4 + wave) * N;
  const float* ratios = a.mc_ratios + (size_t)b * a.ratio_stride;
  float mx = -INFINITY;
  for (int i = lane; i < N; i += 64) {
    const float l = logp_of(a, b, i);
    swr[i] = l;
    slr[i] = l;
    mx = fmaxf(mx, l);
  }
  mx = wave_max_g(mx);
  float ps = 0.f, zs = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float p = expf(swr[i] - mx);
    swr[i] = p;
    ps += p;
    zs += __fmul_rn(ratios[i], p);
  }
  ps = wave_sum_g(ps);
  zs = wave_sum_g(zs);
  const float pbar = __fadd_rn(ps / (float)N, 1e-10f);
  const float zbar = __fadd_rn(zs / (float)N, 1e-10f);
  if (a.diag_rec && lane == 0) a.diag_rec[(size_t)b * RGFM_DIAG_FLOATS + RGFM_DIAG_Z_BAR] = zbar;  // (the untempered value)
  float ws = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float w = __fmul_rn(ratios[i] / zbar, swr[i] / pbar);
    swr[i] = w;
    ws += w;
  }
  ws = __fadd_rn(wave_sum_g(ws), 1e-10f);
  float rsum = 0.f, q = 0.f, npos = 0.f, lmax = -INFINITY;
  for (int i = lane; i < N; i += 64) {
    const float w = swr[i] / ws;
    swr[i] = w;
    rsum += w;
    q = fmaf(w, w, q);
    const float r = ratios[i];
    const float L = r > 0.f ? __fadd_rn(slr[i], logf(r)) : -INFINITY;
    slr[i] = L;
    npos += r > 0.f ? 1.f : 0.f;
    lmax = fmaxf(lmax, L);
  }
  rsum = wave_sum_g(rsum), q = wave_sum_g(q), npos = wave_sum_g(npos), lmax = wave_max_g(lmax);
  const float ess1 = q > 0.f ? __fmul_rn(rsum, rsum) / q : 0.f;
  const float target = fminf(a.ess_min, npos);
  float tau = 1.f;
  // (wave-uniform: every lane holds the same reduced values.  E* <= 1 is met by every row -- an effective sample size
  // is at least 1 -- whatever the rounding of ess1 says)
  if (npos > 0.f && target > 1.f && !(ess1 >= target)) {
    float lo = 0.f, hi = 1.f;
    for (int it = 0; it < ESS_BISECT; ++it) {
      const float mid = __fmul_rn(0.5f, __fadd_rn(lo, hi));
      float s1 = 0.f, s2 = 0.f;
      for (int i = lane; i < N; i += 64) {
        const float L = slr[i];
        const float e = L == -INFINITY ? 0.f : expf(__fmul_rn(mid, __fsub_rn(L, lmax)));
        s1 += e;
        s2 = fmaf(e, e, s2);
      }
      s1 = wave_sum_g(s1), s2 = wave_sum_g(s2);
      if (__fmul_rn(s1, s1) / s2 >= target) lo = mid;  // (s2 >= 1: the sample at the maximum)
      else hi = mid;
    }
    // (lmax is finite here: some r_i > 0, and l_i is finite for finite inputs.  A row whose every l_i is -inf -- a
    // distance that overflows fp32 -- would give d = nan, as it gives nan weights in the sibling)
    tau = lo;
    float s1 = 0.f;
    for (int i = lane; i < N; i += 64) {
      const float L = slr[i];
      const float e = L == -INFINITY ? 0.f : expf(__fmul_rn(tau, __fsub_rn(L, lmax)));
      swr[i] = e;
      s1 += e;
    }
    s1 = wave_sum_g(s1);
    rsum = 0.f;
    for (int i = lane; i < N; i += 64) {
      const float w = swr[i] / s1;
      swr[i] = w;
      rsum += w;
    }
    rsum = wave_sum_g(rsum);
  }
  for (int i = lane; i < N; i += 64) {
    const float w = swr[i];
    a.wbuf[(size_t)b * N + i] = w;
    if (a.weights_out) a.weights_out[(size_t)b * N + i] = w;
  }
  if (lane == 0) {
    a.wsum[b] = rsum;
    if (a.tau_out) a.tau_out[b] = tau;
  }
}

// The guided velocity g_b = sum_i w_bi (m_i - x_b) / c (sample_mnist_svhn.py:157-160) as the fp32 GEMM it is:
//   g_b = (sum_i w_bi m_i  -  x_b sum_i w_bi) / c,   [B, N] x [N, D] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32
// accumulation: the arithmetic of an fmaf chain), then the blend (1 - gamma) v + gamma g and the optional Euler update in
// the epilogue.  The first versions formed every (m_i - x_b) / c w_bi on the vector ALU in the reference's operation
// order: 16 VALU instructions per (row, sample, float4), 110 us at B = 512, N = 256, D = 3072 + 1024 against 7 us of
// matrix work.  Both forms carry the same error: terms of size |m - x| / c summed to a result that may be far smaller.
//
// grid (ceil(B / 32), ceil(dx / 128) + ceil(dy / 128)): both modalities in one launch; workgroup = a 32-row x 128-column output tile, its four
// waves each take a quarter of the MC samples (the two lane halves of a wave: the two halves of that quarter, one
// sample each per MFMA) and add their partial tiles through LDS in wave order.  Lane l supplies W[b0 + l % 32][k] as
// the A element and M[k][d0 + 4 (l % 32) + j] as the B element of column tile j: one float4 of the MC set feeds four
// MFMAs and the lane ends up with four consecutive columns of a row (float4 loads and stores in the epilogue).  A
// row's result depends on its own weights and the MC set only, in an order fixed by N: independent of the batch it is in.
// The blend coefficients of a row with its own strength: gamma = (double)gamma_b * scale, each operation rounded on its
// own (no contraction into 1 - gamma_b scale): the host's rule for GuidanceArgs::g1 / g2 (rgfm_host.h).
__device__ __forceinline__ void row_blend(float gamma_b, double scale, float& g1, float& g2) {
#pragma clang fp contract(off)
  const double gm = (double)gamma_b * scale;
  g1 = (float)(1.0 - gm), g2 = (float)gm;
}

// ROWS: the blend coefficients of a row come from GuidanceArgs::gamma_rows (a strength per sample) instead of g1 / g2;
// the row's entry is fetched in the final epilogue loop, when the accumulators have left the registers for LDS, so the
// main loop and the prefetch block are those of the scalar instantiation.
template <bool W4, bool ROWS>  // W4: N % 32 == 0, a lane's run of samples starts at a multiple of four and its weights arrive as float4
__global__ __launch_bounds__(256, 2) void guid_apply_mfma_kernel(const GuidanceArgs a_in) {
  const GuidanceArgs a = with_schedule(a_in);
  const int nbx = (a.dx + 127) >> 7;  // column blocks of modality x; those of y behind them
  const int part = (int)blockIdx.y >= nbx ? 1 : 0;
  extern __shared__ __attribute__((aligned(16))) float sred[];  // [4 waves][64 accumulators][64 lanes]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hf = lane >> 5;
  const int N = a.N, B = a.B;
  const float* X = part ? a.y : a.x;
  const float* M = part ? a.mc_y1 : a.mc_x1;
  float* V = part ? a.vy : a.vx;
  float* XS = part ? a.y_state : a.x_state;
  const float* XB = part ? a.y_base : a.x_base;  // (null: the update starts from X)
  const int D = part ? a.dy : a.dx;
  const int b0 = blockIdx.x * 32;
  const int d = ((int)blockIdx.y - (part ? nbx : 0)) * 128 + 4 * l31;
  const bool dok = d < D;
  const int KH = (N + 7) >> 3;              // samples per (wave, lane half)
  const int k0 = (wave * 2 + hf) * KH;
  const bool rowok = b0 + l31 < B;
  const float* wb = part && a.wbuf_y ? a.wbuf_y : a.wbuf;  // (cross pairing: the y column blocks have weights of their own)
  const float* wsm = part && a.wbuf_y ? a.wsum_y : a.wsum;
  const float* wrow = wb + (size_t)(rowok ? b0 + l31 : 0) * N;
  const float* mcol = M + (dok ? d : 0);
  constexpr int U = 16;  // samples per group: two groups of registers, one being multiplied (64 MFMAs, 1.7 us) while the other loads
  struct Grp {
    float w[U];
    f32x4 m[U];
  };
  auto load = [&](Grp& g, int s0) {  // (branch-free: clamped addresses, selects)
    if constexpr (W4) {
#pragma unroll
      for (int u = 0; u < U; u += 4) {
        const int s = s0 + u;
        const bool ok = s < KH && rowok;  // (whole quads: KH % 4 == 0)
        const f32x4 wv = *reinterpret_cast<const f32x4*>(wrow + (s < KH ? k0 + s : 0));
        g.w[u] = ok ? wv.x : 0.f, g.w[u + 1] = ok ? wv.y : 0.f, g.w[u + 2] = ok ? wv.z : 0.f, g.w[u + 3] = ok ? wv.w : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int s = s0 + u, k = k0 + s;
      const bool kok = s < KH && k < N;
      const int kc = kok ? k : 0;
      if constexpr (!W4) {
        const float wv = wrow[kc];
        g.w[u] = (kok && rowok) ? wv : 0.f;  // (a sample past the end enters as 0 x finite)
      }
      g.m[u] = *reinterpret_cast<const f32x4*>(mcol + (size_t)kc * D);
    }
  };
  f32x16 acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) acc[j][r] = 0.f;
  auto mult = [&](const Grp& g) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(g.w[u], g.m[u].x, acc[0], 0, 0, 0);
      acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(g.w[u], g.m[u].y, acc[1], 0, 0, 0);
      acc[2] = __builtin_amdgcn_mfma_f32_32x32x2f32(g.w[u], g.m[u].z, acc[2], 0, 0, 0);
      acc[3] = __builtin_amdgcn_mfma_f32_32x32x2f32(g.w[u], g.m[u].w, acc[3], 0, 0, 0);
    }
  };
  Grp g0, g1;  // (no register copies between iterations: a copy would wait for the loads it copies)
  load(g0, 0);
  for (int s0 = 0; s0 < KH; s0 += 2 * U) {
    load(g1, s0 + U);  // (past the end: clamped addresses, zero weights)
    mult(g0);
    if (s0 + 2 * U < KH) load(g0, s0 + 2 * U);
    if (s0 + U < KH) mult(g1);
  }
  // the epilogue's rows of x and v (this wave finishes rows b0 + 8 wave + 4 hf + 0 .. 3), fetched under the exchange of the partial tiles
  f32x4 ex[4], ev[4];
  float esw[4];
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int b = b0 + 8 * wave + 4 * hf + rr;
    const size_t o = (size_t)(b < B ? b : 0) * D + (dok ? d : 0);
    ex[rr] = *reinterpret_cast<const f32x4*>(X + o);
    ev[rr] = *reinterpret_cast<const f32x4*>(V + o);
    esw[rr] = wsm[b < B ? b : 0];
  }
  // partial tiles -> LDS; wave w then owns accumulator rows r = 4w .. 4w + 3: output rows b0 + 8w + 4 (lane / 32) + (r & 3)
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int r = 0; r < 16; ++r) sred[((wave * 64) + j * 16 + r) * 64 + lane] = acc[j][r];
  __syncthreads();
  const float rcden = 1.0f / a.cden;
#pragma unroll
  for (int rr = 0; rr < 4; ++rr) {
    const int r = 4 * wave + rr;
    const int b = b0 + 8 * wave + 4 * hf + rr;
    float c[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      float t = sred[(j * 16 + r) * 64 + lane];
#pragma unroll
      for (int p = 1; p < 4; ++p) t = __fadd_rn(t, sred[((p * 64) + j * 16 + r) * 64 + lane]);
      c[j] = t;
    }
    if (b >= B || !dok) continue;
    const size_t o = (size_t)b * D + d;
    const f32x4 xv = ex[rr], v = ev[rr];
    const float sw = esw[rr];
    float g1 = a.g1, g2 = a.g2;
    if constexpr (ROWS) row_blend(a.gamma_rows[b], a.gamma_scale, g1, g2);  // (b < B here: the load is in bounds)
    // (the blend g1 v + g2 g is written as the fma the compiler contracts it to in the scalar kernel -- fma(g1, v, g2 g)
    // -- so that the per-row instantiations cannot associate it the other way: a row's bits are those of the scalar call)
    f32x4 g, nv;
    g.x = __fmul_rn(__fsub_rn(c[0], __fmul_rn(xv.x, sw)), rcden);
    g.y = __fmul_rn(__fsub_rn(c[1], __fmul_rn(xv.y, sw)), rcden);
    g.z = __fmul_rn(__fsub_rn(c[2], __fmul_rn(xv.z, sw)), rcden);
    g.w = __fmul_rn(__fsub_rn(c[3], __fmul_rn(xv.w, sw)), rcden);
    nv.x = fmaf(g1, v.x, __fmul_rn(g2, g.x));
    nv.y = fmaf(g1, v.y, __fmul_rn(g2, g.y));
    nv.z = fmaf(g1, v.z, __fmul_rn(g2, g.z));
    nv.w = fmaf(g1, v.w, __fmul_rn(g2, g.w));
    if (XS) {
      f32x4 xs = XB ? *reinterpret_cast<const f32x4*>(XB + o) : xv;
      xs.x = __fadd_rn(xs.x, __fmul_rn(nv.x, a.dt));
      xs.y = __fadd_rn(xs.y, __fmul_rn(nv.y, a.dt));
      xs.z = __fadd_rn(xs.z, __fmul_rn(nv.z, a.dt));
      xs.w = __fadd_rn(xs.w, __fmul_rn(nv.w, a.dt));
      *reinterpret_cast<f32x4*>(XS + o) = xs;
    } else {
      *reinterpret_cast<f32x4*>(V + o) = nv;
    }
  }
}

// ---- cross pairing: the importance weights over all N x N pairs (x1_i, y1_j) of the MC set, R_ij = r(x1_i, y1_j)
// (GuidanceArgs::mc_ratios is then the matrix [N][N], x index first).  The Gaussian factor of pair (i, j) is a_i b_j,
//   a_i = exp(lx_i - max lx),  b_j = exp(ly_j - max ly),  lx / ly: the two terms of logp_of, each rounded as there,
// so the reference block on the list of N^2 pairs (p_bar = mean a_i b_j + 1e-10, Z_bar = mean R_ij a_i b_j + 1e-10,
// w_ij = (R_ij / Z_bar)(a_i b_j / p_bar) normalised by its sum + 1e-10) needs only the weights' marginals
//   wx_i = sum_j w_ij ~ a_i u_i,  u = R b        wy_j = sum_i w_ij ~ b_j s_j,  s = R^T a
// and nothing of size N^2 per row.  Three launches: guid_cross_ab_kernel (a, b), guid_cross_prod_kernel (the two
// [B, N] x [N, N] products; a third, q = (R o R) b^2, for the joint ESS when diagnostics are on) and guid_cross_fin_kernel
// (the marginals wx -> wbuf / wsum, wy -> wbuf_y / wsum_y, which guid_apply_mfma_kernel reads per modality).
__global__ __launch_bounds__(256) void guid_cross_ab_kernel(const GuidanceArgs a_in) {
  const GuidanceArgs a = with_schedule(a_in);
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = a.N;
  const int b = blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  float* pa = a.ca + (size_t)b * N;
  float* pb = a.cb + (size_t)b * N;
  float mxa = -INFINITY, mxb = -INFINITY;
  for (int i = lane; i < N; i += 64) {  // (each lane reads back only what it wrote itself)
    double sx = 0.0, sy = 0.0;
    for (int z = 0; z < a.nsx; ++z) sx += a.dist[((size_t)z * a.B + b) * N + i];
    for (int z = a.nsx; z < a.nsx + a.nsy; ++z) sy += a.dist[((size_t)z * a.B + b) * N + i];
    const float lx = __fadd_rn(0.f, __fmul_rn(-0.5f, (float)sx) / a.s2);
    const float ly = __fadd_rn(0.f, __fmul_rn(-0.5f, (float)sy) / a.s2);
    pa[i] = lx, pb[i] = ly;
    mxa = fmaxf(mxa, lx), mxb = fmaxf(mxb, ly);
  }
  mxa = wave_max_g(mxa), mxb = wave_max_g(mxb);
  for (int i = lane; i < N; i += 64) pa[i] = expf(pa[i] - mxa), pb[i] = expf(pb[i] - mxb);
}

// out[b][c] = sum_k A[b][k] M[k][c] on v_mfma_f32_32x32x2_f32 (exact fp32 products, fp32 accumulation; every term is
// non-negative), blockIdx.z picking the product:
//   0: s = a R      (M[k][c] = R[k][c])        1: u = b R^T      (M[k][c] = R[c][k])
//   2: q = b^2 (R o R)^T  (M[k][c] = R[c][k]^2; diagnostics only)
// Workgroup = 32 rows x 128 columns, wave w the 32 x 32 tile of columns 32 w ..; k in chunks of 32 staged through LDS
// (R does not fit: 4 MB at N = 1024), where the transposed products turn R's rows into columns -- both global reads
// run along R's rows.  Rows, columns and k past the end are staged as zeros: any 1 <= N <= 1024, any B.  A row's sum
// runs over k in index order, two terms per MFMA: fixed by N, the same in every batch.
constexpr int XK = 32, XAS = XK + 1, XBS = 128 + 1;
__global__ __launch_bounds__(256) void guid_cross_prod_kernel(const GuidanceArgs a) {
  __shared__ float sA[32 * XAS];
  __shared__ float sB[XK * XBS];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, hf = lane >> 5;
  const int N = a.N, B = a.B;
  const int z = blockIdx.z;
  const int b0 = blockIdx.x * 32, c0 = blockIdx.y * 128;
  const float* A = z == 0 ? a.ca : a.cb;
  const float* R = a.mc_ratios;
  float* out = z == 0 ? a.cs : z == 1 ? a.cu : a.cq;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = 0; k0 < N; k0 += XK) {
    __syncthreads();
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int e = tid + 256 * j, k = e & 31, row = e >> 5;
      const bool ok = b0 + row < B && k0 + k < N;
      float v = A[ok ? (size_t)(b0 + row) * N + k0 + k : 0];
      v = ok ? v : 0.f;
      sA[row * XAS + k] = z == 2 ? v * v : v;
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int e = tid + 256 * j;
      const int k = z == 0 ? e >> 7 : e & 31, c = z == 0 ? e & 127 : e >> 5;
      const bool ok = k0 + k < N && c0 + c < N;
      const size_t g = z == 0 ? (size_t)(k0 + k) * N + c0 + c : (size_t)(c0 + c) * N + k0 + k;
      float v = R[ok ? g : 0];
      v = ok ? v : 0.f;
      sB[k * XBS + c] = z == 2 ? v * v : v;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < XK / 2; ++kk) {
      const int k = 2 * kk + hf;
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(sA[l31 * XAS + k], sB[k * XBS + wave * 32 + l31], acc, 0, 0, 0);
    }
  }
  const int c = c0 + wave * 32 + l31;
#pragma unroll
  for (int r = 0; r < 16; ++r) {  // accumulator r of a lane: row 8 (r / 4) + 4 (lane / 32) + r % 4, column lane % 32
    const int b = b0 + 8 * (r >> 2) + 4 * hf + (r & 3);
    if (b < B && c < N) out[(size_t)b * N + c] = acc[r];
  }
}

// The marginal weights of one row per wave, from a, b, u, s: with E = a.u (= b.s up to rounding)
//   p_bar = (sum a)(sum b) / N^2 + 1e-10,  Z_bar = E / N^2 + 1e-10,
//   wx_i = (u_i / Z_bar)(a_i / p_bar) / (their sum + 1e-10),  wy_j = (s_j / Z_bar)(b_j / p_bar) / (their sum + 1e-10)
// -- the operation order of guid_weights_kernel with u / s in the ratio's place; each marginal is normalised by its own
// sum (the two sums are the same number, sum_ij w_ij, up to rounding).  A zero row (column) of R gives u_i (s_j) = 0 and
// a weight of exactly 0.  Diagnostics: Z_bar, the range over the 2N marginal weights and the joint effective sample
// size (sum_ij w_ij)^2 / sum_ij w_ij^2 = (a.u)^2 / (a^2 . q), formed from u / Z_bar and q / Z_bar^2 so that the
// scale of R cancels before anything is squared.
__global__ __launch_bounds__(256) void guid_cross_fin_kernel(const GuidanceArgs a) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int N = a.N;
  const int b = blockIdx.x * 4 + wave;
  if (b >= a.B) return;
  const size_t o = (size_t)b * N;
  const float *pa = a.ca + o, *pb = a.cb + o, *pu = a.cu + o, *ps = a.cs + o;
  float *wx = a.wbuf + o, *wy = a.wbuf_y + o;
  float sa = 0.f, sb = 0.f, e = 0.f;
  for (int i = lane; i < N; i += 64) {
    sa += pa[i], sb += pb[i];
    e += __fmul_rn(pa[i], pu[i]);
  }
  sa = wave_sum_g(sa), sb = wave_sum_g(sb), e = wave_sum_g(e);
  const float nn = (float)N * (float)N;
  const float pbar = __fadd_rn(__fmul_rn(sa, sb) / nn, 1e-10f);
  const float zbar = __fadd_rn(e / nn, 1e-10f);
  float tx = 0.f, ty = 0.f;
  for (int i = lane; i < N; i += 64) {
    const float vx = __fmul_rn(pu[i] / zbar, pa[i] / pbar), vy = __fmul_rn(ps[i] / zbar, pb[i] / pbar);
    wx[i] = vx, wy[i] = vy;
    tx += vx, ty += vy;
  }
  tx = __fadd_rn(wave_sum_g(tx), 1e-10f), ty = __fadd_rn(wave_sum_g(ty), 1e-10f);
  float rx = 0.f, ry = 0.f, mx = -INFINITY, mn = INFINITY;
  for (int i = lane; i < N; i += 64) {
    const float vx = wx[i] / tx, vy = wy[i] / ty;
    wx[i] = vx, wy[i] = vy;
    if (a.weights_out) a.weights_out[o + i] = vx;
    if (a.weights_out_y) a.weights_out_y[o + i] = vy;
    rx += vx, ry += vy;
    mx = fmaxf(mx, fmaxf(vx, vy)), mn = fminf(mn, fminf(vx, vy));
  }
  rx = wave_sum_g(rx), ry = wave_sum_g(ry);
  if (lane == 0) a.wsum[b] = rx, a.wsum_y[b] = ry;
  if (!a.diag_rec) return;
  const float* pq = a.cq + o;
  float es = 0.f, fs = 0.f;
  for (int i = lane; i < N; i += 64) {
    es += __fmul_rn(pa[i], pu[i] / zbar);
    fs += __fmul_rn(__fmul_rn(pa[i], pa[i]), (pq[i] / zbar) / zbar);
  }
  es = wave_sum_g(es), fs = wave_sum_g(fs);
  mx = wave_max_g(mx);
#pragma unroll
  for (int s = 32; s > 0; s >>= 1) mn = fminf(mn, __shfl_xor(mn, s));
  if (lane == 0) {
    float* r = a.diag_rec + (size_t)b * RGFM_DIAG_FLOATS;
    r[RGFM_DIAG_ESS] = fs > 0.f ? es * es / fs : 0.f;
    r[RGFM_DIAG_W_MAX] = mx;
    r[RGFM_DIAG_W_MIN] = mn;
    r[RGFM_DIAG_Z_BAR] = zbar;
  }
}

void launch_guid_cross_weights(const GuidanceArgs& a, hipStream_t s) {  // (needs the distances only: no velocity)
  const dim3 rows((a.B + 3) / 4);
  hipLaunchKernelGGL(guid_cross_ab_kernel, rows, dim3(256), 0, s, a);
  hipLaunchKernelGGL(guid_cross_prod_kernel, dim3((a.B + 31) / 32, (a.N + 127) / 128, a.diag_rec ? 3 : 2), dim3(256), 0, s, a);
  hipLaunchKernelGGL(guid_cross_fin_kernel, rows, dim3(256), 0, s, a);
}

// ---- diagnostics (opt-in: launched only for a caller that passes a record buffer; include/rgfm.h, RGFM_DIAG_*)
__device__ __forceinline__ float wave_min_g(float v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fminf(v, __shfl_xor(v, o));
  return v;
}

// Row statistics of the step's importance weights w [B][N] (GuidanceArgs::wbuf), one wave per row as guid_weights_kernel:
// lane l adds samples l, l + 64, ... in index order, the 64 partials meet in the xor butterfly -- an order fixed by N
// alone, the same on every lane.  ess = (sum w)^2 / sum w^2; a row whose weights are all zero (every ratio zero) has
// ess 0.  N < 64: the idle lanes hold the identities (0, -inf, +inf).
__global__ __launch_bounds__(256) void guid_diag_wstats_kernel(const float* __restrict__ w, int B, int N, float* __restrict__ rec) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  const float* wr = w + (size_t)b * N;
  float s = 0.f, q = 0.f, mx = -INFINITY, mn = INFINITY;
  for (int i = lane; i < N; i += 64) {
    const float v = wr[i];
    s += v;
    q = fmaf(v, v, q);
    mx = fmaxf(mx, v);
    mn = fminf(mn, v);
  }
  s = wave_sum_g(s), q = wave_sum_g(q), mx = wave_max_g(mx), mn = wave_min_g(mn);
  if (lane == 0) {
    float* r = rec + (size_t)b * RGFM_DIAG_FLOATS;
    r[RGFM_DIAG_ESS] = q > 0.f ? s * s / q : 0.f;
    r[RGFM_DIAG_W_MAX] = mx;
    r[RGFM_DIAG_W_MIN] = mn;
  }
}

// rec[b][slot] = |v_b|_2 for v [B][D], D % 4 == 0: one wave per row, lane l squares float4s l, l + 64, ... into four
// running sums (one per component), adds them pairwise and the 64 partials in the xor butterfly: an order fixed by D.
__global__ __launch_bounds__(256) void guid_diag_rownorm_kernel(const float* __restrict__ v, int B, int D, float* __restrict__ rec, int slot) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int b = blockIdx.x * 4 + wave;
  if (b >= B) return;
  const f32x4* r = reinterpret_cast<const f32x4*>(v + (size_t)b * D);
  float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
  for (int i = lane; i < (D >> 2); i += 64) {
    const f32x4 a = r[i];
    s0 = fmaf(a.x, a.x, s0), s1 = fmaf(a.y, a.y, s1), s2 = fmaf(a.z, a.z, s2), s3 = fmaf(a.w, a.w, s3);
  }
  const float s = wave_sum_g((s0 + s1) + (s2 + s3));
  if (lane == 0) rec[(size_t)b * RGFM_DIAG_FLOATS + slot] = sqrtf(s);
}

void launch_diag_wstats(const float* w, int B, int N, float* rec, hipStream_t s) {
  hipLaunchKernelGGL(guid_diag_wstats_kernel, dim3((B + 3) / 4), dim3(256), 0, s, w, B, N, rec);
}
void launch_diag_rownorm(const float* v, int B, int D, float* rec, int slot, hipStream_t s) {
  hipLaunchKernelGGL(guid_diag_rownorm_kernel, dim3((B + 3) / 4), dim3(256), 0, s, v, B, D, rec, slot);
}

void launch_guid_logp(const GuidanceArgs& a, hipStream_t s) {
  dim3 g1((a.B + 31) / 32, (a.N + 63) / 64, a.nsx + a.nsy);
  hipLaunchKernelGGL(guid_logp_kernel, g1, dim3(256), 0, s, a);
}

int guid_apply_init() {  // (64 KB of dynamic LDS)
  int rc = 0;
  for (const void* k : {reinterpret_cast<const void*>(&guid_apply_mfma_kernel<true, false>), reinterpret_cast<const void*>(&guid_apply_mfma_kernel<false, false>),
                        reinterpret_cast<const void*>(&guid_apply_mfma_kernel<true, true>), reinterpret_cast<const void*>(&guid_apply_mfma_kernel<false, true>)})
    rc |= (int)hipFuncSetAttribute(k, hipFuncAttributeMaxDynamicSharedMemorySize, 64 * 1024);
  // (the floor's weights kernel: two [4][N] arrays, 128 KB of the CU's 160 at n_mc = 4096 -- no smaller cap than its sibling's)
  rc |= (int)hipFuncSetAttribute(reinterpret_cast<const void*>(&guid_weights_ess_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, 128 * 1024);
  return rc;
}

void launch_guid_weights(const GuidanceArgs& a, hipStream_t s) {  // (needs the distances only: no velocity)
  hipLaunchKernelGGL(guid_weights_kernel, dim3((a.B + 3) / 4), dim3(256), (size_t)4 * a.N * sizeof(float), s, a);
}

void launch_guid_weights_ess(const GuidanceArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(guid_weights_ess_kernel, dim3((a.B + 3) / 4), dim3(256), (size_t)8 * a.N * sizeof(float), s, a);
}

void launch_guid_apply(const GuidanceArgs& a, hipStream_t s) {
  const size_t lds = (size_t)4 * 64 * 64 * sizeof(float);
  const dim3 grid((a.B + 31) / 32, (a.dx + 127) / 128 + (a.dy + 127) / 128);
  if (a.gamma_rows) {  // (a strength per row: the ROWS instantiations)
    if (a.N % 32 == 0) hipLaunchKernelGGL((guid_apply_mfma_kernel<true, true>), grid, dim3(256), lds, s, a);
    else hipLaunchKernelGGL((guid_apply_mfma_kernel<false, true>), grid, dim3(256), lds, s, a);
    return;
  }
  if (a.N % 32 == 0) hipLaunchKernelGGL((guid_apply_mfma_kernel<true, false>), grid, dim3(256), lds, s, a);
  else hipLaunchKernelGGL((guid_apply_mfma_kernel<false, false>), grid, dim3(256), lds, s, a);
}

// x <- x + v * dt (mul, then add: two roundings like the reference's x_t + v * dt)
__global__ void euler_kernel(float* x, const float* v, size_t n, float dt) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    x[i] = __fadd_rn(x[i], __fmul_rn(v[i], dt));
}

// Per-step scalars of the guidance block for steps step_begin .. step_begin + ns - 1: the reference's Python-double
// arithmetic (sample_mnist_svhn.py:115,127,135,159: t = step * dt, sigma_t = 1 - t + eps), the same IEEE double
// operations the host path performs, rounded to fp32 where a tensor op consumes them.
__global__ void guid_schedule_kernel(float* sched, int step_begin, int ns, int num_steps) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= ns) return;
  const double dtd = 1.0 / (double)num_steps;
  const double t = (double)(step_begin + i) * dtd;
  const double eps = 1e-3;
  const double sigma_t = 1.0 - t + eps;
  sched[4 * i] = (float)t, sched[4 * i + 1] = (float)(sigma_t * sigma_t), sched[4 * i + 2] = (float)(1.0 - t + eps), sched[4 * i + 3] = 0.f;
}
void launch_guid_schedule(float* sched, int step_begin, int ns, int num_steps, hipStream_t s) {
  hipLaunchKernelGGL(guid_schedule_kernel, dim3((ns + 255) / 256), dim3(256), 0, s, sched, step_begin, ns, num_steps);
}

__global__ void step_inc_kernel(int* step) { *step += 1; }
void launch_step_inc(int* step, hipStream_t s) { hipLaunchKernelGGL(step_inc_kernel, dim3(1), dim3(1), 0, s, step); }

void launch_euler(float* x, const float* v, size_t n, float dt, hipStream_t s) {
  const int blocks = (int)((n + 255) / 256 < 2048 ? (n + 255) / 256 : 2048);
  hipLaunchKernelGGL(euler_kernel, dim3(blocks), dim3(256), 0, s, x, v, n, dt);
}

}  // namespace rgfm
