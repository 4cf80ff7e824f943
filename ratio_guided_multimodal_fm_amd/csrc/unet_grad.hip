// unet_grad.hip -- training pass of FlexibleUNet (reference src/models/unet_flexible.py:39-261): the forward that keeps
// what the backward needs, and the backward itself, on exact fp32 arithmetic ("Training").
//
// Every tensor of this path is NCHW fp32.  All convolutions -- forward, data gradient and weight gradient, 3x3 and 1x1,
// stride 1, stride 2 (Downsample) and nearest-x2-then-3x3 (Upsample) -- are one implicit GEMM on
// v_mfma_f32_32x32x2_f32 (ug_igemm_kernel), instantiated three times with different operand gathers:
//   forward  C[co][pixel]      = sum_(ci,tap)   W[co][ci][tap]   X[b][ci][src(pixel, tap)]
//   dgrad    C[ci][in-pixel]   = sum_(co,tap)   W[co][ci][tap]   dY[b][co][dst(in-pixel, tap)]   (stride 2: the
//            output pixel exists only where (in + pad - tap) is even -- the zero insertion is implicit in the gather)
//   wgrad    C[co][(ci,tap)]   = sum_(b,pixel)  dY[b][co][pixel] X[b][ci][src(pixel, tap)]
// The weight gradient's K axis (B*H*W, up to 131 072) is split across workgroups: each writes its own partial slice and
// ug_reduce_kernel adds the slices in split order, so no float atomics and bitwise-reproducible gradients.  Every
// other reduction (GroupNorm statistics, dgamma / dbeta, bias, time path) is a fixed-order loop or LDS tree as well.
// The same kernel knows 4x4 taps (stride 2, pad 1): FlowMatchingModel's ConvTranspose2d(4, 2, 1) layers are the data
// gradient / forward / weight gradient of that conv with the roles of x and dy exchanged (api_fmnet_train.cpp).
//
// GroupNorm + SiLU (+ dropout) of a conv's input is applied by ug_gn_act_kernel into a transient buffer right before
// the conv that consumes it (and again in the backward): the saved state holds only the pre-norm tensors and the
// group (mean, rstd) pairs.
#include <cstring>

#include "rgfm_device.h"
#include "train_device.h"

namespace rgfm {

// ------------------------------------------------------------------ implicit GEMM
// Block tile 64 (M) x 64 (N), K staged 16 at a time; four waves, one 32x32 accumulator each (ug_mfma_chunk,
// train_device.h).  Each thread stages 4 consecutive k of ONE row of A and ONE row (column) of B.
// (ky, kx) of tap tp: 1 tap (pad 0), 3 x 3 or 4 x 4 (pad 1)
__device__ __forceinline__ void ug_tap(int taps, int tp, int& ky, int& kx) {
  if (taps == 16) ky = tp >> 2, kx = tp & 3;
  else if (taps == 9) ky = tp / 3, kx = tp - 3 * (tp / 3);
  else ky = kx = 0;
}
__device__ __forceinline__ void ug_pix(int n, int HW, int W, int& b, int& y, int& x) {
  b = n / HW;
  const int p = n - b * HW;
  y = p / W;
  x = p - y * W;
}

template <int OP>
__global__ __launch_bounds__(256) void ug_igemm_kernel(UgConv a) {
  __shared__ __attribute__((aligned(16))) float sA[64 * LDP];
  __shared__ __attribute__((aligned(16))) float sB[64 * LDP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int l31 = lane & 31, h = lane >> 5;
  const int wm = wave & 1, wn = wave >> 1;
  const int m0 = blockIdx.y * 64, n0 = blockIdx.x * 64;
  const int row = tid >> 2, q = tid & 3;
  const int taps = a.taps, pad = taps == 1 ? 0 : 1;
  const int HWo = a.Ho * a.Wo, HWc = a.Hc * a.Wc, HWs = a.Hs * a.Ws;
  int M, N, K;
  if (OP == 0) M = a.Cout, N = a.B * HWo, K = a.Cin * taps;
  else if (OP == 1) M = a.Cin, N = a.B * HWc, K = a.Cout * taps;
  else M = a.Cout, N = a.Cin * taps, K = a.B * HWo;
  const int kbeg = blockIdx.z * a.kps;
  const int kend = min(K, kbeg + a.kps);
  // per-thread fixed parts of the gathers
  const int am = m0 + row, bn = n0 + row;
  int pb = 0, py = 0, px = 0;  // OP 0: output pixel of column bn; OP 1: conv-input pixel of column bn
  int wci = 0, wky = 0, wkx = 0;  // OP 2: (ci, tap) of column bn
  if (OP == 0 && bn < N) ug_pix(bn, HWo, a.Wo, pb, py, px);
  if (OP == 1 && bn < N) ug_pix(bn, HWc, a.Wc, pb, py, px);
  if (OP == 2 && bn < N) {
    wci = bn / taps;
    const int tp = bn - wci * taps;
    ug_tap(taps, tp, wky, wkx);
  }
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int k0 = kbeg; k0 < kend; k0 += KC) {
    float va[4], vb[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int k = k0 + q * 4 + j;
      float x = 0.f, y = 0.f;
      if (k < kend) {
        if (OP == 0) {
          if (am < M) x = a.w[(size_t)am * K + k];
          if (bn < N) {
            const int ci = k / taps, tp = k - ci * taps;
            int ky, kx;
            ug_tap(taps, tp, ky, kx);
            const int cy = py * a.stride - pad + ky, cx = px * a.stride - pad + kx;
            if (cy >= 0 && cy < a.Hc && cx >= 0 && cx < a.Wc) {
              const int sy = a.up ? cy >> 1 : cy, sx = a.up ? cx >> 1 : cx;
              y = a.x[((size_t)pb * a.Cin + ci) * HWs + sy * a.Ws + sx];
            }
          }
        } else if (OP == 1) {
          const int co = k / taps, tp = k - co * taps;
          if (am < M) x = a.w[((size_t)co * a.Cin + am) * taps + tp];
          if (bn < N) {
            int ky, kx;
            ug_tap(taps, tp, ky, kx);
            const int ny = py + pad - ky, nx = px + pad - kx;  // = oy * stride
            if (ny >= 0 && nx >= 0) {
              const int oy = ny / a.stride, ox = nx / a.stride;
              if (oy * a.stride == ny && ox * a.stride == nx && oy < a.Ho && ox < a.Wo)
                y = a.dy[((size_t)pb * a.Cout + co) * HWo + oy * a.Wo + ox];
            }
          }
        } else {
          const int b = k / HWo, p = k - b * HWo;
          if (am < M) x = a.dy[((size_t)b * a.Cout + am) * HWo + p];
          if (bn < N) {
            const int oy = p / a.Wo, ox = p - oy * a.Wo;
            const int cy = oy * a.stride - pad + wky, cx = ox * a.stride - pad + wkx;
            if (cy >= 0 && cy < a.Hc && cx >= 0 && cx < a.Wc) {
              const int sy = a.up ? cy >> 1 : cy, sx = a.up ? cx >> 1 : cx;
              y = a.x[((size_t)b * a.Cin + wci) * HWs + sy * a.Ws + sx];
            }
          }
        }
      }
      va[j] = x, vb[j] = y;
    }
    ug_mfma_chunk(sA, sB, row, q, va, row, q, vb, wm, wn, l31, h, acc);
  }
  // C/D: column n = lane & 31 (consecutive lanes -> consecutive pixels), row m = (r & 3) + 8 (r >> 2) + 4 h
  const int n = n0 + wn * 32 + l31;
  if (n >= N) return;
  if (OP == 2) {
    float* out = a.part + (size_t)blockIdx.z * M * N;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
      if (m < M) out[(size_t)m * N + n] = acc[r];
    }
    return;
  }
  int b, y, x;
  if (OP == 0) ug_pix(n, HWo, a.Wo, b, y, x);
  else ug_pix(n, HWc, a.Wc, b, y, x);
  const int pix = OP == 0 ? y * a.Wo + x : y * a.Wc + x;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int m = m0 + wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * h;
    if (m >= M) continue;
    if (OP == 0) {
      const size_t o = ((size_t)b * a.Cout + m) * HWo + pix;
      float v = acc[r];
      if (a.bias) v += a.bias[m];
      if (a.temb) v += a.temb[(size_t)b * a.Cout + m];
      if (a.res) v += a.res[o];
      a.out[o] = v;
    } else {
      // data gradient, split by channel range into the two sources of a concatenated input
      float* dst;
      size_t o;
      int accum;
      if (m < a.C0) dst = a.out, o = ((size_t)b * a.C0 + m) * HWc + pix, accum = a.acc0;
      else dst = a.out1, o = ((size_t)b * (a.Cin - a.C0) + (m - a.C0)) * HWc + pix, accum = a.acc1;
      const float v = a.dbias ? acc[r] + a.dbias[m] : acc[r];
      dst[o] = accum ? dst[o] + v : v;
    }
  }
}

void launch_ug_conv(const UgConv& c, int op, hipStream_t s) {
  int M, N;
  if (op == 0) M = c.Cout, N = c.B * c.Ho * c.Wo;
  else if (op == 1) M = c.Cin, N = c.B * c.Hc * c.Wc;
  else M = c.Cout, N = c.Cin * c.taps;
  const dim3 grid((N + 63) / 64, (M + 63) / 64, op == 2 ? c.splits : 1);
  if (op == 0) hipLaunchKernelGGL(ug_igemm_kernel<0>, grid, dim3(256), 0, s, c);
  else if (op == 1) hipLaunchKernelGGL(ug_igemm_kernel<1>, grid, dim3(256), 0, s, c);
  else hipLaunchKernelGGL(ug_igemm_kernel<2>, grid, dim3(256), 0, s, c);
}

// out[i] = sum over z of part[z][i], z ascending
__global__ void ug_reduce_kernel(const float* part, int splits, size_t n, float* out) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    float v = 0.f;
    for (int z = 0; z < splits; ++z) v += part[(size_t)z * n + i];
    out[i] = v;
  }
}
void launch_ug_reduce(const float* part, int splits, size_t n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ug_reduce_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 2048)), dim3(256), 0, s, part,
                     splits, n, out);
}

// db[c] = sum over (b, pixel) of dy[b][c][pixel]; one workgroup per channel
__global__ __launch_bounds__(256) void ug_bias_grad_kernel(const float* dy, int B, int C, int HW, float* db) {
  __shared__ float red[256];
  const int c = blockIdx.x;
  float v = 0.f;
  for (int b = 0; b < B; ++b)
    for (int p = threadIdx.x; p < HW; p += 256) v += dy[((size_t)b * C + c) * HW + p];
  v = ug_block_sum(v, red);
  if (threadIdx.x == 0) db[c] = v;
}
void launch_ug_bias_grad(const float* dy, int B, int C, int HW, float* db, hipStream_t s) {
  hipLaunchKernelGGL(ug_bias_grad_kernel, dim3(C), dim3(256), 0, s, dy, B, C, HW, db);
}

// ------------------------------------------------------------------ GroupNorm (+ SiLU, + dropout)
__device__ __forceinline__ float ug_src(const float* s0, const float* s1, int C0, int C1, int b, int c, int HW, int p) {
  return c < C0 ? s0[((size_t)b * C0 + c) * HW + p] : s1[((size_t)b * C1 + (c - C0)) * HW + p];
}

// mr[b][g] = (mean, rstd) of group g of cat(s0, s1)[b]; one workgroup per (b, g); two passes (eps 1e-5, biased var)
__global__ __launch_bounds__(256) void ug_gn_stats_kernel(const float* s0, const float* s1, int C0, int C1, int HW,
                                                          int groups, float* mr) {
  __shared__ float red[256];
  const int b = blockIdx.x / groups, g = blockIdx.x % groups;
  const int cg = (C0 + C1) / groups, n = cg * HW;
  float v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) v += ug_src(s0, s1, C0, C1, b, g * cg + i / HW, HW, i % HW);
  const float mean = ug_block_sum(v, red) / (float)n;
  v = 0.f;
  for (int i = threadIdx.x; i < n; i += 256) {
    const float d = ug_src(s0, s1, C0, C1, b, g * cg + i / HW, HW, i % HW) - mean;
    v += d * d;
  }
  const float var = ug_block_sum(v, red) / (float)n;
  if (threadIdx.x == 0) mr[2 * blockIdx.x] = mean, mr[2 * blockIdx.x + 1] = 1.0f / sqrtf(var + 1e-5f);
}
void launch_ug_gn_stats(const float* s0, const float* s1, int C0, int C1, int B, int HW, int groups, float* mr,
                        hipStream_t s) {
  hipLaunchKernelGGL(ug_gn_stats_kernel, dim3(B * groups), dim3(256), 0, s, s0, s1, C0, C1, HW, groups, mr);
}

// out[b][c][p] = cat(s0, s1), optionally normalised (mr != null), SiLU'd and dropped (drop_p > 0)
__global__ void ug_gn_act_kernel(UgAct a) {
  const int C = a.C0 + a.C1, cg = C / max(a.groups, 1);
  const size_t total = (size_t)a.B * C * a.HW;
  float drop_p;
  uint64_t seed;
  ug_drop_params(a.drop_hdr, drop_p, seed);
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = i % a.HW;
    const size_t r = i / a.HW;
    const int c = r % C, b = r / C;
    float v = ug_src(a.s0, a.s1, a.C0, a.C1, b, c, a.HW, p);
    if (a.mr) {
      const float* m = a.mr + 2 * (b * a.groups + c / cg);
      v = ug_silu(a.gamma[c] * ((v - m[0]) * m[1]) + a.beta[c]);
      if (drop_p > 0.f) v = ug_keep(seed, a.block, (uint32_t)i, drop_p) ? v * keep_scale : 0.f;
    }
    a.out[i] = v;
  }
}
void launch_ug_gn_act(const UgAct& a, hipStream_t s) {
  const size_t total = (size_t)a.B * (a.C0 + a.C1) * a.HW;
  hipLaunchKernelGGL(ug_gn_act_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s, a);
}

// Backward of out = drop(silu(gamma xhat + beta)): a.out is dL/d(out) (read), the input gradient goes to d0 / d1 (the
// channel ranges of the two sources; acc0 / acc1: add instead of overwrite), and pg / pb [B][C] receive the per-sample
// dgamma / dbeta partials (summed over b by ug_colsum_kernel; pg null: not wanted, the data-only walk of rgfm_unet_vjp).
// One workgroup per (b, g).
__global__ __launch_bounds__(256) void ug_gn_act_bwd_kernel(UgAct a, const float* dout, float* d0, float* d1, int acc0,
                                                            int acc1, float* pg, float* pb) {
  __shared__ float red[256];
  const int b = blockIdx.x / a.groups, g = blockIdx.x % a.groups;
  const int C = a.C0 + a.C1, cg = C / a.groups, HW = a.HW;
  const float mean = a.mr[2 * blockIdx.x], rstd = a.mr[2 * blockIdx.x + 1];
  float drop_p;
  uint64_t seed;
  ug_drop_params(a.drop_hdr, drop_p, seed);
  const float keep_scale = drop_p > 0.f ? 1.0f / (1.0f - drop_p) : 1.0f;
  // dy = d(gamma xhat + beta); recomputed per pass (no scratch)
  auto dyf = [&](int c, int p, float& xh) {
    const float v = ug_src(a.s0, a.s1, a.C0, a.C1, b, c, HW, p);
    xh = (v - mean) * rstd;
    const size_t i = ((size_t)b * C + c) * HW + p;
    float go = dout[i];
    if (drop_p > 0.f) go = ug_keep(seed, a.block, (uint32_t)i, drop_p) ? go * keep_scale : 0.f;
    return go * ug_dsilu(a.gamma[c] * xh + a.beta[c]);
  };
  float s1 = 0.f, s2 = 0.f;
  for (int cc = 0; cc < cg; ++cc) {
    const int c = g * cg + cc;
    float sg = 0.f, sb = 0.f;
    for (int p = threadIdx.x; p < HW; p += 256) {
      float xh;
      const float dy = dyf(c, p, xh);
      sb += dy, sg += dy * xh;
    }
    sg = ug_block_sum(sg, red);
    sb = ug_block_sum(sb, red);
    if (threadIdx.x == 0 && pg) pg[(size_t)b * C + c] = sg, pb[(size_t)b * C + c] = sb;
    s1 += a.gamma[c] * sb;  // sum of dy gamma
    s2 += a.gamma[c] * sg;  // sum of dy gamma xhat
  }
  const float inv_n = 1.0f / (float)(cg * HW);
  const float m1 = s1 * inv_n, m2 = s2 * inv_n;
  for (int cc = 0; cc < cg; ++cc) {
    const int c = g * cg + cc;
    for (int p = threadIdx.x; p < HW; p += 256) {
      float xh;
      const float dy = dyf(c, p, xh);
      const float dx = rstd * (dy * a.gamma[c] - m1 - xh * m2);
      if (c < a.C0) {
        float* o = d0 + ((size_t)b * a.C0 + c) * HW + p;
        *o = acc0 ? *o + dx : dx;
      } else {
        float* o = d1 + ((size_t)b * a.C1 + (c - a.C0)) * HW + p;
        *o = acc1 ? *o + dx : dx;
      }
    }
  }
}
void launch_ug_gn_act_bwd(const UgAct& a, const float* dout, float* d0, float* d1, int acc0, int acc1, float* pg,
                          float* pb, hipStream_t s) {
  hipLaunchKernelGGL(ug_gn_act_bwd_kernel, dim3(a.B * a.groups), dim3(256), 0, s, a, dout, d0, d1, acc0, acc1, pg, pb);
}

// out[c] = sum over r (ascending) of in[r][c]
__global__ void ug_colsum_kernel(const float* in, int rows, int cols, float* out) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= cols) return;
  float v = 0.f;
  for (int r = 0; r < rows; ++r) v += in[(size_t)r * cols + c];
  out[c] = v;
}
void launch_ug_colsum(const float* in, int rows, int cols, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ug_colsum_kernel, dim3((cols + 255) / 256), dim3(256), 0, s, in, rows, cols, out);
}

// out[r] = sum over p (ascending) of in[r][p]  (d temb_out[b][c] = sum over the pixels of dh[b][c])
__global__ void ug_rowsum_kernel(const float* in, int rows, int n, float* out) {
  const int r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= rows) return;
  float v = 0.f;
  for (int p = 0; p < n; ++p) v += in[(size_t)r * n + p];
  out[r] = v;
}
void launch_ug_rowsum(const float* in, int rows, int n, float* out, hipStream_t s) {
  hipLaunchKernelGGL(ug_rowsum_kernel, dim3((rows + 255) / 256), dim3(256), 0, s, in, rows, n, out);
}

// ------------------------------------------------------------------ small dense layers of the time path
// y[r][o] = b[o] + sum_i f(x[r][i]) W[o][i], f = SiLU when silu_in
__global__ void ug_linear_kernel(const float* x, const float* w, const float* bias, float* y, int rows, int in, int out,
                                 int silu_in) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * out) return;
  const int r = i / out, o = i % out;
  float v = 0.f;
  for (int k = 0; k < in; ++k) {
    const float xv = x[(size_t)r * in + k];
    v += (silu_in ? ug_silu(xv) : xv) * w[(size_t)o * in + k];
  }
  y[i] = v + bias[o];
}
void launch_ug_linear(const float* x, const float* w, const float* b, float* y, int rows, int in, int out, int silu_in,
                      hipStream_t s) {
  hipLaunchKernelGGL(ug_linear_kernel, dim3((rows * out + 255) / 256), dim3(256), 0, s, x, w, b, y, rows, in, out,
                     silu_in);
}
// dW[o][i] = sum_r dy[r][o] f(x[r][i]); db[o] = sum_r dy[r][o]
__global__ void ug_linear_wgrad_kernel(const float* dy, const float* x, int rows, int in, int out, int silu_in,
                                       float* dw, float* db) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= out * (in + 1)) return;
  if (i >= out * in) {
    const int o = i - out * in;
    float v = 0.f;
    for (int r = 0; r < rows; ++r) v += dy[(size_t)r * out + o];
    db[o] = v;
    return;
  }
  const int o = i / in, k = i % in;
  float v = 0.f;
  for (int r = 0; r < rows; ++r) {
    const float xv = x[(size_t)r * in + k];
    v += dy[(size_t)r * out + o] * (silu_in ? ug_silu(xv) : xv);
  }
  dw[i] = v;
}
void launch_ug_linear_wgrad(const float* dy, const float* x, int rows, int in, int out, int silu_in, float* dw,
                            float* db, hipStream_t s) {
  const int n = out * (in + 1);
  hipLaunchKernelGGL(ug_linear_wgrad_kernel, dim3((n + 255) / 256), dim3(256), 0, s, dy, x, rows, in, out, silu_in, dw,
                     db);
}
// dx[r][i] (+)= sum_o dy[r][o] W[o][i]
__global__ void ug_linear_dgrad_kernel(const float* dy, const float* w, int rows, int in, int out, float* dx, int acc) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= rows * in) return;
  const int r = i / in, k = i % in;
  float v = 0.f;
  for (int o = 0; o < out; ++o) v += dy[(size_t)r * out + o] * w[(size_t)o * in + k];
  dx[i] = acc ? dx[i] + v : v;
}
void launch_ug_linear_dgrad(const float* dy, const float* w, int rows, int in, int out, float* dx, int acc,
                            hipStream_t s) {
  hipLaunchKernelGGL(ug_linear_dgrad_kernel, dim3((rows * in + 255) / 256), dim3(256), 0, s, dy, w, rows, in, out, dx,
                     acc);
}
// g[i] *= silu'(x[i])
__global__ void ug_dsilu_kernel(float* g, const float* x, int n) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) g[i] *= ug_dsilu(x[i]);
}
void launch_ug_dsilu(float* g, const float* x, int n, hipStream_t s) {
  hipLaunchKernelGGL(ug_dsilu_kernel, dim3((n + 255) / 256), dim3(256), 0, s, g, x, n);
}
// emb[b][0:half] = cos(t_b f), emb[b][half:2 half] = sin(t_b f)  (unet_flexible.py:16-36), t_b = t[t_count == 1 ? 0 : b]
__global__ void ug_sincos_kernel(const float* t, int t_count, const float* freqs, int B, int mc, float* emb) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int half = mc / 2;
  if (i >= B * mc) return;
  const int b = i / mc, j = i % mc;
  const float tv = t[t_count == 1 ? 0 : b];
  float v = 0.f;
  if (j < 2 * half) {
    const float arg = tv * freqs[j % half];
    v = j < half ? cosf(arg) : sinf(arg);
  }
  emb[i] = v;
}
void launch_ug_sincos(const float* t, int t_count, const float* freqs, int B, int mc, float* emb, hipStream_t s) {
  hipLaunchKernelGGL(ug_sincos_kernel, dim3((B * mc + 255) / 256), dim3(256), 0, s, t, t_count, freqs, B, mc, emb);
}

// ------------------------------------------------------------------ elementwise
// dx[b][c][y][x] += sum of the four dU[b][c][2y + i][2x + j]  (the nearest-x2 upsample's gradient)
__global__ void ug_pool2_add_kernel(const float* du, float* dx, int BC, int H, int W) {
  const size_t total = (size_t)BC * H * W;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int x = i % W;
    const size_t r = i / W;
    const int y = r % H;
    const size_t bc = r / H;
    const float* u = du + (bc * 2 * H + 2 * y) * 2 * W + 2 * x;
    dx[i] += (u[0] + u[1]) + (u[2 * W] + u[2 * W + 1]);
  }
}
void launch_ug_pool2_add(const float* du, float* dx, int BC, int H, int W, hipStream_t s) {
  const size_t total = (size_t)BC * H * W;
  hipLaunchKernelGGL(ug_pool2_add_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s,
                     du, dx, BC, H, W);
}
// dst (+)= src; with a second destination: the channel ranges [0, C0) / [C0, C) of a [B][C][HW] source
__global__ void ug_split_add_kernel(const float* src, float* d0, float* d1, int B, int C0, int C1, int HW) {
  const int C = C0 + C1;
  const size_t total = (size_t)B * C * HW;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int p = i % HW;
    const size_t r = i / HW;
    const int c = r % C, b = r / C;
    if (c < C0) d0[((size_t)b * C0 + c) * HW + p] += src[i];
    else d1[((size_t)b * C1 + (c - C0)) * HW + p] += src[i];
  }
}
void launch_ug_split_add(const float* src, float* d0, float* d1, int B, int C0, int C1, int HW, hipStream_t s) {
  const size_t total = (size_t)B * (C0 + C1) * HW;
  hipLaunchKernelGGL(ug_split_add_kernel, dim3((unsigned)std::min<size_t>((total + 255) / 256, 4096)), dim3(256), 0, s,
                     src, d0, d1, B, C0, C1, HW);
}
// mask[i] = 1 / 0: the keep decisions of ResBlock `block` over n elements (rgfm_unet_dropout_mask)
__global__ void ug_mask_kernel(float* out, size_t n, uint64_t seed, int block, float p) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
    out[i] = ug_keep(seed, block, (uint32_t)i, p) ? 1.f : 0.f;
}
void launch_ug_mask(float* out, size_t n, uint64_t seed, int block, float p, hipStream_t s) {
  hipLaunchKernelGGL(ug_mask_kernel, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, s, out, n,
                     seed, block, p);
}
// the saved state's dropout header {p_drop bits, seed lo, seed hi}: written by the training forward, read on the device
// by every dropout site of the forward and of the backward (whose C signature carries neither value)
__global__ void ug_header_kernel(unsigned* hdr, unsigned w0, unsigned w1, unsigned w2) {
  if (threadIdx.x == 0) hdr[0] = w0, hdr[1] = w1, hdr[2] = w2, hdr[3] = 0u;
}
void launch_ug_header(unsigned* hdr, float p, uint64_t seed, hipStream_t s) {
  unsigned pw;
  std::memcpy(&pw, &p, 4);
  hipLaunchKernelGGL(ug_header_kernel, dim3(1), dim3(64), 0, s, hdr, pw, (unsigned)seed, (unsigned)(seed >> 32));
}

}  // namespace rgfm
