// Joint exact-GP posterior covariance at new inputs (eval mode) for gfx950, phase 2.
//
// Replaces, per window b, the dense evaluation of upstream
// models/exact_prediction_strategies.py exact_predictive_covar (reached from reference
// denoising_model/GPModel.py:10-13 in eval mode):
//   Sigma = K(xs, xs) - V^T V,   V = L^{-1} K*   (N x Ns)
// Phase 1 (the V-storing variants of the posterior kernels, gpk_posterior.hip /
// gpk_exact_large.hip) leaves V in the caller's workspace, row-major (B, N, vs) with the row
// stride vs = Ns rounded up to 64, followed by the training mean of x / l that centred its
// Gram (B x 64 floats), together with mean and var. This file is the SYRK-shaped phase 2.
//
// Design: one workgroup of 4 waves per (window, 64 x 64 output tile with tile row <= tile
// column); wave w owns the 16-column strip w of the tile, four 16 x 16 accumulators down the
// tile's 64 rows.
//   K(xs_i, xs_j): the test inputs of both tile sides are staged in LDS scaled by 1 / l and
//     centred by the TRAINING mean (phase 1's own, read back from the workspace: no workgroup
//     here walks the training inputs), the Gram runs on fp32 MFMA,
//     d2 = |a|^2 + |b|^2 - 2 a.b clamped at 0, k = s2 exp2(-0.5 log2(e) d2).
//   V^T V: the two 64-column panels of V are staged through LDS in 32-row chunks (the next
//     chunk's global loads in flight under this chunk's MFMAs) and accumulated with
//     mfma_f32_16x16x4f32 in ascending k. Everything is exact fp32: Sigma is a difference of
//     near-equal numbers near the training inputs. The V chunks reuse the LDS of the staged
//     inputs (dead once K is in registers): 36 KB per workgroup, four workgroups per CU.
// The tile and its mirror are stored from the same registers (cov[i][j] == cov[j][i] bitwise;
// a diagonal tile stores only its strict upper half and mirrors it), and the diagonal is
// phase 1's var (diag(cov) == var bitwise). No atomics, fixed summation order: deterministic.
// Rows >= N and columns >= Ns of the workspace are never used (masked to 0 on load).
#include "gpk_common.h"
#include "gpk_posterior_cov.h"

namespace {

constexpr int kCovTile = 64;          // output tile edge
constexpr int kCovKC = 32;            // rows of V per LDS chunk
constexpr int kCovVS = kCovTile + 16; // LDS row stride of a V chunk: ds_read_b32 banks are
                                      // (a / 4) % 32 per 32-lane half; the half's two k rows
                                      // land 16 banks apart
constexpr int kCovXS = 64 + 4;        // LDS row stride of the staged test inputs (as post_lds_layout)

// VAR = false: the exact posterior above. VAR = true: the covariance of a variational q(f),
// cov = K(x, x) + jitter I + A^T diag(vstd^2 - 1) A from phase 1's A = L^{-1} K_ZX
// (gpk_variational_cov.hip; workspace rows M, row stride as, then the window's own mean of
// x / l): the weight vstd_m^2 - 1 is folded into the I-side panel as a chunk is staged, the
// product is added, and the diagonal is computed here (K_ii = s2 exactly, + jitter). Output o
// of a batched launch is blockIdx.y.
// gpk_vcc_syrk_kernel (gpk_var_chol_cov.hip) is this tile with a +-1 row weight over 2 M rows: a
// shared body takes 2 - 4 SGPRs off all three kernels, so edit them together.
template <bool VAR>
__global__ __launch_bounds__(256) void gpk_post_cov_kernel(GpkCovArgsOf<VAR> a) {
  __shared__ float mu[64];
  __shared__ float lsc[64];
  __shared__ float nI[kCovTile];
  __shared__ float nJ[kCovTile];
  // the staged inputs of both tile sides; after the Gram, the two V chunks
  __shared__ __attribute__((aligned(16))) float buf[2 * kCovTile * kCovXS];
  static_assert(2 * kCovKC * kCovVS <= 2 * kCovTile * kCovXS, "V chunks must fit the input staging");
  float* xI = buf;
  float* xJ = buf + kCovTile * kCovXS;
  float* vI = buf;
  float* vJ = buf + kCovKC * kCovVS;

  int N, Ns;
  if constexpr (VAR) { N = a.M; Ns = a.N; } else { N = a.N; Ns = a.Ns; }
  const int D = a.D;
  const int T = (Ns + kCovTile - 1) / kCovTile;
  const int P = T * (T + 1) / 2;
  // XCD-aware order: the tile pairs of one window go to the same XCD (shared L2 for V)
  const int total = a.B * P;
  int id = blockIdx.x;
  if ((total & 7) == 0) id = (id & 7) * (total >> 3) + (id >> 3);
  const int b = id / P;
  int ti, tj;
  tile_of(id - b * P, T, ti, tj);   // ti <= tj
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  const int c = lane & 15, g = lane >> 4;
  const int D4 = (D + 3) & ~3;

  const float* hyp = a.hyp;
  const float* Xs;
  const float* Vb;
  const float* mup;
  const float* wstd = nullptr;
  int vs;
  if constexpr (VAR) {
    const size_t o = blockIdx.y;
    hyp += o * (size_t)(4 + 2 * D);
    Xs = a.X + o * (size_t)a.x_stride + (size_t)b * Ns * D;
    Vb = a.A + o * (size_t)a.ws_stride + (size_t)b * N * a.as;
    mup = a.A + o * (size_t)a.ws_stride + (size_t)a.B * N * a.as;
    wstd = a.vstd + o * (size_t)N;
    vs = a.as;
  } else {
    hyp += (long long)b * a.hyp_stride;  // this window's hyper vector (stride 0: shared)
    Xs = a.Xs + (size_t)b * Ns * D;
    Vb = a.V + (size_t)b * N * a.vs;
    mup = a.mu;
    vs = a.vs;
  }
  const float s2 = hyp[0];

  // ---- the first V chunk's loads go out before anything else (one f32x4 per panel, thread
  //      and 16-row half chunk: row = 16 h + tid / 16, columns 4 (tid % 16) ..)
  const int vr = tid >> 4, vc = 4 * (tid & 15);
  f32x4 ra[2], rb[2];
  float rw[2];
  auto vload = [&](int k0) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int row = k0 + 16 * h + vr;
      const size_t off = (size_t)(row < N ? row : 0) * vs;
      if constexpr (VAR) rw[h] = wstd[row < N ? row : 0];
      ra[h] = *(const f32x4*)&Vb[off + kCovTile * ti + vc];
      rb[h] = *(const f32x4*)&Vb[off + kCovTile * tj + vc];
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        if (row >= N || kCovTile * ti + vc + t >= Ns) ra[h][t] = 0.f;
        if (row >= N || kCovTile * tj + vc + t >= Ns) rb[h][t] = 0.f;
      }
    }
  };
  vload(0);

  // ---- phase 1's training mean of x / l, and the lengthscales
  if (tid < 64) {
    mu[tid] = tid < D ? mup[(size_t)b * 64 + tid] : 0.f;
    if constexpr (VAR) lsc[tid] = tid < D ? hyp[4 + D + tid] : 1.f;
    else lsc[tid] = tid < D ? hyp[3 + (a.n_ls > 1 ? tid : 0)] : 1.f;
  }
  lds_barrier();
  // ---- both sides' test inputs, scaled, centred, zero padded
  for (int e = tid; e < kCovTile * 64; e += 256) {
    const int r = e >> 6, d = e & 63;
    const int ci = kCovTile * ti + r, cj = kCovTile * tj + r;
    const bool okd = d < D;
    const float vi = Xs[(okd && ci < Ns) ? (size_t)ci * D + d : 0];
    const float vj = Xs[(okd && cj < Ns) ? (size_t)cj * D + d : 0];
    const float l = lsc[d], m = mu[d];
    xI[r * kCovXS + d] = (okd && ci < Ns) ? vi / l - m : 0.f;
    xJ[r * kCovXS + d] = (okd && cj < Ns) ? vj / l - m : 0.f;
  }
  lds_barrier();
  if (tid < 2 * kCovTile) {
    const float* x = (tid < kCovTile ? xI : xJ) + (tid & 63) * kCovXS;
    float s = 0.f;
    for (int d = 0; d < D4; ++d) s = __builtin_fmaf(x[d], x[d], s);
    (tid < kCovTile ? nI : nJ)[tid & 63] = s;
  }
  lds_barrier();

  // ---- K(xs_I, xs_J) for this wave's strip: acc layout, reg r = tile row 16 it + 4 g + r,
  //      column 16 w + c
  constexpr float nhalf_log2e = -0.72134752044448170f;
  f32x4 Kt[4];
  {
    f32x4 G[4];
#pragma unroll
    for (int it = 0; it < 4; ++it) G[it] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int d0 = 0; d0 < D4; d0 += 4) {
      const float bj = xJ[(16 * w + c) * kCovXS + d0 + g];
#pragma unroll
      for (int it = 0; it < 4; ++it)
        G[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(xI[(16 * it + c) * kCovXS + d0 + g], bj, G[it], 0, 0, 0);
    }
    const float nj = nJ[16 * w + c];
#pragma unroll
    for (int it = 0; it < 4; ++it)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const float d2 = __builtin_fmaxf(nI[16 * it + 4 * g + r] + nj - 2.f * G[it][r], 0.f);
        Kt[it][r] = s2 * __builtin_amdgcn_exp2f(d2 * nhalf_log2e);
      }
  }

  // ---- V_I^T V_J over the N rows, 32 at a time, ascending k
  f32x4 acc[4];
#pragma unroll
  for (int it = 0; it < 4; ++it) acc[it] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int k0 = 0; k0 < N; k0 += kCovKC) {
    lds_barrier();   // the previous chunk's reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      if constexpr (VAR) *(f32x4*)&vI[(16 * h + vr) * kCovVS + vc] = ra[h] * (rw[h] * rw[h] - 1.f);
      else *(f32x4*)&vI[(16 * h + vr) * kCovVS + vc] = ra[h];
      *(f32x4*)&vJ[(16 * h + vr) * kCovVS + vc] = rb[h];
    }
    lds_barrier();
    if (k0 + kCovKC < N) vload(k0 + kCovKC);
#pragma unroll
    for (int kk = 0; kk < kCovKC; kk += 4) {
      const float bj = vJ[(kk + g) * kCovVS + 16 * w + c];
#pragma unroll
      for (int it = 0; it < 4; ++it)
        acc[it] = __builtin_amdgcn_mfma_f32_16x16x4f32(vI[(kk + g) * kCovVS + 16 * it + c], bj, acc[it], 0, 0, 0);
    }
  }

  // ---- Sigma tile and its mirror from the same registers; the diagonal is phase 1's var
  //      (variational mode: s2 + jitter + the tile's own weighted sum of squares)
  float* Cb = a.cov + (size_t)b * Ns * Ns;
  if constexpr (VAR) Cb += (size_t)blockIdx.y * a.B * Ns * Ns;
  const float* varb = nullptr;
  float dg = 0.f;
  if constexpr (VAR) dg = s2 + hyp[2];
  else varb = a.var + (size_t)b * Ns;
  const int col = kCovTile * tj + 16 * w + c;
#pragma unroll
  for (int it = 0; it < 4; ++it)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int row = kCovTile * ti + 16 * it + 4 * g + r;
      if (row >= Ns || col >= Ns) continue;
      if (row < col) {
        const float v = VAR ? Kt[it][r] + acc[it][r] : Kt[it][r] - acc[it][r];
        Cb[(size_t)row * Ns + col] = v;
        Cb[(size_t)col * Ns + row] = v;
      } else if (row == col) {
        Cb[(size_t)row * Ns + col] = VAR ? dg + acc[it][r] : varb[row];
      }
    }
}

}  // namespace

int gpk_post_cov_vstride(int Ns) { return (Ns + kCovTile - 1) / kCovTile * kCovTile; }

size_t gpk_post_cov_ws_floats(int B, int N, int Ns) {
  return (size_t)B * N * gpk_post_cov_vstride(Ns) + (size_t)B * 64;
}

int gpk_launch_exact_posterior_cov(const GpkPostCovArgs& a, hipStream_t stream) {
  const long long T = (a.Ns + kCovTile - 1) / kCovTile;
  const long long grid = (long long)a.B * (T * (T + 1) / 2);
  if (grid > 0x7fffffff) return -7;
  hipLaunchKernelGGL(gpk_post_cov_kernel<false>, dim3((unsigned)grid), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}

int gpk_launch_variational_cov_phase2(const GpkVarCovArgs& a, int O, hipStream_t stream) {
  const long long T = (a.N + kCovTile - 1) / kCovTile;
  const long long grid = (long long)a.B * (T * (T + 1) / 2);
  if (grid > 0x7fffffff) return -9;
  hipLaunchKernelGGL(gpk_post_cov_kernel<true>, dim3((unsigned)grid, O), dim3(256), 0, stream, a);
  return (int)hipGetLastError();
}
