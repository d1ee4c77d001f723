// Adjoint of the batched Cholesky root fused with sampling (gpk_mvn_root.hip), for gfx950.
//
// Replaces the autograd backward of upstream psd_safe_cholesky (torch.linalg.cholesky's
// cholesky_backward) and of MultivariateNormal.rsample's mean + R eps matmul, which train.py:166
// runs through the skip-input draw of denoising_model/DeepGP.py:62-64.
//
// Per matrix b, from the forward's factor R and the upstream gradients gR, gsamples:
//   Rbar = tril(gR) + tril(sum_s gsamples[s] (x) eps[s])
//   P    = Phi(R^T Rbar)          Phi: lower triangle, diagonal halved
//   Sbar = W^T P W                W = R^{-1}
//   dcov = (Sbar + Sbar^T) / 2    dmean = sum_s gsamples[s]
//
// Design: one workgroup of 4 waves per matrix, as the forward. The lower tile triangle of R,
// later of W, lives in LDS as packed 16 x 16 tiles (T (T + 1) / 2 KB, T = ceil(n / 16), padded
// with an identity diagonal); P and M = P W stream through one tile triangle of the caller's
// workspace (one slice per matrix, written and read by the same workgroup only). Every tile is
// held in acc layout (gpk_common.h), element (row, col) at float 4 (16 (row / 4) + col) + row % 4,
// so mma_tn(Q, P) = Q^T P on mfma_f32_16x16x4f32 needs no transposes, and a phase that needs
// the other side of a factor finds it after an in-place transposition of the LDS tiles:
//   1. P^T_ij = sum_{k >= i} Rbar_kj^T R_ki   (Rbar tiles formed in registers from gR, gsamples,
//      eps; Phi on the diagonal tiles)                                  -> workspace
//   2. the LDS tiles are transposed in place (now R^T, the forward's layout); the diagonal
//      tiles are inverted by forward substitution (lane c owns column c)
//   3. block rows i = 1 .. T - 1:  W_ij = -W_ii sum_{j <= k < i} R_ik W_kj, in place
//   4. M_ij = sum_{j <= k <= i} P_ik W_kj, in place over P (a wave owns whole block rows and
//      goes j upwards, so it never reads a tile it has overwritten)
//   5. dcov_ij = (sum_{k >= i} W_ki^T M_kj + sum_{k >= i} M_ki^T W_kj) / 2 for i >= j, stored
//      to (i, j) and mirrored to (j, i); a diagonal tile is mirrored from its own lower
//      triangle through LDS: dcov is symmetric bit for bit.
// All arithmetic fp32 in a fixed order, no atomics: two launches give the same bits.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"

#include <mutex>

namespace {

GPK_DEVICE int rg_el(int row, int col) { return 4 * (16 * (row >> 2) + col) + (row & 3); }
GPK_DEVICE int rg_tile(int i, int j) { return (i * (i + 1) / 2 + j) * 256; }
// Block row i of phase 4 -> wave: 0 1 2 3 3 2 1 0 ... (row i costs ~ i^2 / 2 tile products)
GPK_DEVICE int rg_row_owner(int i) { return (i & 4) ? 3 - (i & 3) : (i & 3); }

// Barrier that also orders the workgroup's global stores in front of its later global loads
// (P and M go through the workspace between phases).
GPK_DEVICE void ws_barrier() { __syncthreads(); }

__global__ __launch_bounds__(256) void gpk_mvn_root_grad_kernel(const float* __restrict__ R,
                                                                const float* __restrict__ gR,
                                                                const float* __restrict__ gs,
                                                                const float* __restrict__ eps, int B, int n,
                                                                int S, float* ws, float* __restrict__ dcov,
                                                                float* __restrict__ dmean) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = (n + 15) >> 4, np = 16 * T, TT = T * (T + 1) / 2;
  float* tiles = lds;
  float* side = lds + (size_t)TT * 256;   // max(T, 4) tiles: inverses of the diagonal tiles; later scratch
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const size_t b = blockIdx.x;
  const float* Rb = R + b * (size_t)n * n;
  const float* gRb = gR != nullptr ? gR + b * (size_t)n * n : nullptr;
  float* Pw = ws + b * (size_t)TT * 256;
  float* out = dcov + b * (size_t)n * n;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  if (dmean != nullptr) {
    for (int i = tid; i < n; i += 256) {
      float acc = 0.f;
      for (int s = 0; s < S; ++s) acc += gs[((size_t)s * B + b) * (size_t)n + i];
      dmean[b * (size_t)n + i] = acc;
    }
  }
  if (gRb == nullptr && S == 0) {   // uniform: no gradient arrives
    for (int e = tid; e < n * n; e += 256) out[e] = 0.f;
    return;
  }

  // ---- lower triangle of R into the packed tiles, identity padding
  for (int e = tid; e < np * np; e += 256) {
    const int i = e / np, j = e - i * np;
    if ((j >> 4) > (i >> 4)) continue;
    float v;
    if (i < n && j < n) v = j <= i ? Rb[(size_t)i * n + j] : 0.f;
    else v = i == j ? 1.f : 0.f;
    tiles[rg_tile(i >> 4, j >> 4) + rg_el(i & 15, j & 15)] = v;
  }
  lds_barrier();

  // ---- 1. P^T_ij = sum_k Rbar_kj^T R_ki, tiles round-robin over the waves
  {
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int j = 0; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        const int col = 16 * j + c;
        f32x4 acc = zero4;
        for (int k = i; k < T; ++k) {
          f32x4 rb = zero4;
          const int row0 = 16 * k + 4 * g;
          if (col < n) {
            for (int s = 0; s < S; ++s) {
              const size_t base = ((size_t)s * B + b) * (size_t)n;
              const float e = eps[base + col];
#pragma unroll
              for (int r = 0; r < 4; ++r)
                if (row0 + r < n) rb[r] = __builtin_fmaf(gs[base + row0 + r], e, rb[r]);
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int row = row0 + r;
              if (row < n && col <= row) {
                if (gRb != nullptr) rb[r] += gRb[(size_t)row * n + col];
              } else {
                rb[r] = 0.f;
              }
            }
          }
          acc = mma_tn(rb, *(const f32x4*)&tiles[rg_tile(k, i) + 4 * lane], acc);
        }
        if (i == j) {   // Phi on P_ii: acc holds P_ii^T, keep its upper triangle, halve the diagonal
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 4 * g + r;
            acc[r] = a < c ? acc[r] : (a == c ? 0.5f * acc[r] : 0.f);
          }
        }
        *(f32x4*)&Pw[rg_tile(i, j) + 4 * lane] = acc;
      }
    }
  }
  lds_barrier();

  // ---- 2. transpose every LDS tile in place; invert the diagonal tiles
  for (int t = w; t < TT; t += 4) {
    float* X = tiles + (size_t)t * 256;
    const f32x4 v = *(const f32x4*)&X[4 * lane];
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) X[rg_el(c, 4 * g + r)] = v[r];
  }
  lds_barrier();
  for (int k = w; k < T; k += 4) {
    float* Dk = tiles + rg_tile(k, k);   // holds R_kk^T: R_kk[i][j] at rg_el(j, i)
    float x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float s = i == c ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < i; ++j) s = __builtin_fmaf(-Dk[rg_el(j, i)], x[j], s);
      x[i] = s / Dk[rg_el(i, i)];
    }
    wave_lds_sync();
    const f32x4 o = pick_group4(x, g);   // W_kk[4g + r][c]
    *(f32x4*)&Dk[4 * lane] = o;
    float* It = side + (size_t)k * 256;  // W_kk^T
#pragma unroll
    for (int r = 0; r < 4; ++r) It[rg_el(c, 4 * g + r)] = o[r];
  }

  // ---- 3. W_ij = -W_ii sum_{j <= k < i} R_ik W_kj, block rows top down, in place
  for (int i = 1; i < T; ++i) {
    lds_barrier();   // rows < i (and the diagonal inverses) are complete
    f32x4 y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = w + 4 * q;
      y[q] = zero4;
      if (j < i) {
        for (int k = j; k < i; ++k)
          y[q] = mma_tn(*(const f32x4*)&tiles[rg_tile(i, k) + 4 * lane],
                        *(const f32x4*)&tiles[rg_tile(k, j) + 4 * lane], y[q]);
      }
    }
    lds_barrier();   // every read of row i's R tiles is done
    const f32x4 wi = *(const f32x4*)&side[(size_t)i * 256 + 4 * lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = w + 4 * q;
      if (j < i) *(f32x4*)&tiles[rg_tile(i, j) + 4 * lane] = mma_tn(wi, -y[q], zero4);
    }
  }
  ws_barrier();   // W complete in LDS; P complete in the workspace

  // ---- 4. M_ij = sum_{j <= k <= i} P_ik W_kj, in place over P; a wave owns whole block rows
  for (int i = 0; i < T; ++i) {
    if (rg_row_owner(i) != w) continue;
    for (int j = 0; j <= i; ++j) {
      f32x4 acc = zero4;
      for (int k = j; k <= i; ++k)
        acc = mma_tn(*(const f32x4*)&Pw[rg_tile(i, k) + 4 * lane],
                     *(const f32x4*)&tiles[rg_tile(k, j) + 4 * lane], acc);
      *(f32x4*)&Pw[rg_tile(i, j) + 4 * lane] = acc;
    }
  }
  ws_barrier();

  // ---- 5. dcov_ij = (W^T M + (W^T M)^T)_ij / 2 for i >= j, mirrored to (j, i)
  {
    float* mine = side + (size_t)w * 256;
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int j = 0; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        f32x4 a1 = zero4, a2 = zero4;
        for (int k = i; k < T; ++k) {
          a1 = mma_tn(*(const f32x4*)&tiles[rg_tile(k, i) + 4 * lane],
                      *(const f32x4*)&Pw[rg_tile(k, j) + 4 * lane], a1);
          a2 = mma_tn(*(const f32x4*)&Pw[rg_tile(k, i) + 4 * lane],
                      *(const f32x4*)&tiles[rg_tile(k, j) + 4 * lane], a2);
        }
        f32x4 v = 0.5f * (a1 + a2);
        const int col = 16 * j + c;
        if (i == j) {
          wave_lds_sync();   // the previous diagonal tile's reads of the scratch are done
          *(f32x4*)&mine[4 * lane] = v;
          wave_lds_sync();
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 4 * g + r;
            v[r] = mine[a >= c ? rg_el(a, c) : rg_el(c, a)];
          }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * i + 4 * g + r;
          if (row < n && col < n) {
            out[(size_t)row * n + col] = v[r];
            if (i != j) out[(size_t)col * n + row] = v[r];
          }
        }
      }
    }
  }
}

}  // namespace

size_t gpk_mvn_root_grad_ws_floats(int B, int n) {
  const size_t T = ((size_t)n + 15) / 16;
  return (size_t)B * (T * (T + 1) / 2) * 256;
}

int gpk_launch_mvn_root_grad(const float* R, const float* gR, const float* gsamples, const float* eps, int B,
                             int n, int S, float* ws, float* dcov, float* dmean, hipStream_t stream) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_mvn_root_grad_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipGetLastError();
  });
  const int T = (n + 15) / 16;
  const size_t lds = ((size_t)(T * (T + 1) / 2) + (size_t)(T > 4 ? T : 4)) * 256 * sizeof(float);
  hipLaunchKernelGGL(gpk_mvn_root_grad_kernel, dim3((unsigned)B), dim3(256), lds, stream, R, gR, gsamples, eps,
                     B, n, S, ws, dcov, dmean);
  return (int)hipGetLastError();
}
