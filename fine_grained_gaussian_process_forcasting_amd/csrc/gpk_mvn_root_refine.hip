// One refinement step of the fp32 Cholesky root of gpk_mvn_root.hip, for gfx950: the accurate
// factor the adjoint (gpk_mvn_root_grad.hip) needs when the jitter ladder had to engage.
//
// Per matrix b, from Sigma, the jitter and the forward's factor R (R R^T ~ Sigma + jitter I):
//   E  = Sigma + jitter I - R R^T      (residual accumulated in fp64, stored in fp32)
//   Y  = W E W^T,  W = R^{-1}          R1 = R + R Phi(Y)     Phi: lower triangle, diagonal halved
// (Sigma + jitter I = R (I + Y) R^T and chol(I + Y) = I + Phi(Y) + O(Y^2).) A near-singular
// Sigma leaves the fp32 factor cond * 2^-24 from the true one, which its gradient amplifies
// once more; R1 is as close as fp32 storage allows.
//
// Design: one workgroup of 4 waves per matrix, the tile layout, the in-place transposition and
// the in-place block inversion of gpk_mvn_root_grad.hip (acc layout, mma_tn(Q, P) = Q^T P).
// E (lower tiles; an upper tile is read transposed), Z = W E (lower tiles) and G = Phi(Y) go
// through the caller's workspace, two tile triangles per matrix. Fixed order, no atomics.
#include "gpk_common.h"

#include <mutex>

namespace {

GPK_DEVICE int rf_el(int row, int col) { return 4 * (16 * (row >> 2) + col) + (row & 3); }
GPK_DEVICE int rf_tile(int i, int j) { return (i * (i + 1) / 2 + j) * 256; }
// A stored tile of X read as the tile of X^T.
GPK_DEVICE f32x4 rf_load_t(const float* tile, int g, int c) {
  f32x4 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = tile[rf_el(c, 4 * g + r)];
  return v;
}

GPK_DEVICE void rf_transpose_tiles(float* tiles, int TT, int w, int lane, int g, int c) {
  for (int t = w; t < TT; t += 4) {
    float* X = tiles + (size_t)t * 256;
    const f32x4 v = *(const f32x4*)&X[4 * lane];
    wave_lds_sync();
#pragma unroll
    for (int r = 0; r < 4; ++r) X[rf_el(c, 4 * g + r)] = v[r];
  }
}

__global__ __launch_bounds__(256) void gpk_mvn_root_refine_kernel(const float* __restrict__ cov,
                                                                  const float* __restrict__ R, int B, int n,
                                                                  float jitter, float* ws,
                                                                  float* __restrict__ Rout) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = (n + 15) >> 4, np = 16 * T, TT = T * (T + 1) / 2;
  float* tiles = lds;
  float* side = lds + (size_t)TT * 256;   // T tiles: transposed inverses of the diagonal tiles
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const size_t b = blockIdx.x;
  const float* Ab = cov + b * (size_t)n * n;
  const float* Rb = R + b * (size_t)n * n;
  float* Ew = ws + b * (size_t)TT * 512;   // E, later G^T
  float* Zw = Ew + (size_t)TT * 256;       // Z = W E
  float* out = Rout + b * (size_t)n * n;
  const f32x4 zero4 = {0.f, 0.f, 0.f, 0.f};

  // ---- lower triangle of R into the packed tiles, identity padding; zero upper triangle of Rout
  for (int e = tid; e < np * np; e += 256) {
    const int i = e / np, j = e - i * np;
    if ((j >> 4) > (i >> 4)) {
      if (i < n && j < n) out[(size_t)i * n + j] = 0.f;
      continue;
    }
    float v;
    if (i < n && j < n) v = j <= i ? Rb[(size_t)i * n + j] : 0.f;
    else v = i == j ? 1.f : 0.f;
    tiles[rf_tile(i >> 4, j >> 4) + rf_el(i & 15, j & 15)] = v;
  }
  lds_barrier();

  // ---- E_ij = Sigma_ij + jitter I - sum_{k <= j} R_ik R_jk^T in fp64, i >= j
  {
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int j = 0; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        double acc[4] = {0.0, 0.0, 0.0, 0.0};
        for (int k = 0; k <= j; ++k) {
          const float* Tik = tiles + rf_tile(i, k);
          const float* Tjk = tiles + rf_tile(j, k);
          for (int cc = 0; cc < 16; ++cc) {
            const double rj = (double)Tjk[rf_el(c, cc)];
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[r] = __builtin_fma((double)Tik[rf_el(4 * g + r, cc)], rj, acc[r]);
          }
        }
        f32x4 e4 = zero4;
        const int col = 16 * j + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * i + 4 * g + r;
          if (row < n && col < n) {
            const float a = col <= row ? Ab[(size_t)row * n + col] : Ab[(size_t)col * n + row];
            e4[r] = (float)((double)a + (row == col ? (double)jitter : 0.0) - acc[r]);
          }
        }
        *(f32x4*)&Ew[rf_tile(i, j) + 4 * lane] = e4;
      }
    }
  }
  lds_barrier();

  // ---- W = R^{-1} in place (as gpk_mvn_root_grad.hip, phases 2 and 3)
  rf_transpose_tiles(tiles, TT, w, lane, g, c);
  lds_barrier();
  for (int k = w; k < T; k += 4) {
    float* Dk = tiles + rf_tile(k, k);   // holds R_kk^T
    float x[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      float s = i == c ? 1.f : 0.f;
#pragma unroll
      for (int j = 0; j < i; ++j) s = __builtin_fmaf(-Dk[rf_el(j, i)], x[j], s);
      x[i] = s / Dk[rf_el(i, i)];
    }
    wave_lds_sync();
    const f32x4 o = pick_group4(x, g);
    *(f32x4*)&Dk[4 * lane] = o;
    float* It = side + (size_t)k * 256;
#pragma unroll
    for (int r = 0; r < 4; ++r) It[rf_el(c, 4 * g + r)] = o[r];
  }
  for (int i = 1; i < T; ++i) {
    lds_barrier();
    f32x4 y[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = w + 4 * q;
      y[q] = zero4;
      if (j < i) {
        for (int k = j; k < i; ++k)
          y[q] = mma_tn(*(const f32x4*)&tiles[rf_tile(i, k) + 4 * lane],
                        *(const f32x4*)&tiles[rf_tile(k, j) + 4 * lane], y[q]);
      }
    }
    lds_barrier();
    const f32x4 wi = *(const f32x4*)&side[(size_t)i * 256 + 4 * lane];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int j = w + 4 * q;
      if (j < i) *(f32x4*)&tiles[rf_tile(i, j) + 4 * lane] = mma_tn(wi, -y[q], zero4);
    }
  }
  lds_barrier();
  rf_transpose_tiles(tiles, TT, w, lane, g, c);   // now W_ij^T: mma_tn(tile(i, k), X) = W_ik X
  __syncthreads();                                // and E is visible to every wave

  // ---- Z_il = sum_{k <= i} W_ik E_kl for i >= l
  {
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int l = 0; l <= i; ++l, ++cnt) {
        if ((cnt & 3) != w) continue;
        f32x4 acc = zero4;
        for (int k = 0; k <= i; ++k) {
          const f32x4 e4 = k >= l ? *(const f32x4*)&Ew[rf_tile(k, l) + 4 * lane] : rf_load_t(Ew + rf_tile(l, k), g, c);
          acc = mma_tn(*(const f32x4*)&tiles[rf_tile(i, k) + 4 * lane], e4, acc);
        }
        *(f32x4*)&Zw[rf_tile(i, l) + 4 * lane] = acc;
      }
    }
  }
  __syncthreads();

  // ---- G^T_ij = Phi(Y)^T_ij, Y^T_ij = sum_{l <= j} W_jl Z_il^T for i >= j; over E
  {
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int j = 0; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        f32x4 acc = zero4;
        for (int l = 0; l <= j; ++l)
          acc = mma_tn(*(const f32x4*)&tiles[rf_tile(j, l) + 4 * lane], rf_load_t(Zw + rf_tile(i, l), g, c), acc);
        if (i == j) {
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int a = 4 * g + r;
            acc[r] = a < c ? acc[r] : (a == c ? 0.5f * acc[r] : 0.f);
          }
        }
        *(f32x4*)&Ew[rf_tile(i, j) + 4 * lane] = acc;
      }
    }
  }
  __syncthreads();

  // ---- R1_ij = R_ij + sum_{j <= k <= i} R_ik G_kj
  {
    int cnt = 0;
    for (int i = 0; i < T; ++i) {
      for (int j = 0; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        f32x4 acc = zero4;
        const int rrow = 16 * i + c;
        for (int k = j; k <= i; ++k) {
          f32x4 rt = zero4;   // R_ik^T
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int rcol = 16 * k + 4 * g + r;
            if (rrow < n && rcol <= rrow) rt[r] = Rb[(size_t)rrow * n + rcol];
          }
          acc = mma_tn(rt, rf_load_t(Ew + rf_tile(k, j), g, c), acc);
        }
        const int col = 16 * j + c;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int row = 16 * i + 4 * g + r;
          if (row < n && col < n) out[(size_t)row * n + col] = col <= row ? Rb[(size_t)row * n + col] + acc[r] : 0.f;
        }
      }
    }
  }
}

}  // namespace

size_t gpk_mvn_root_refine_ws_floats(int B, int n) {
  const size_t T = ((size_t)n + 15) / 16;
  return (size_t)B * (T * (T + 1) / 2) * 512;
}

int gpk_launch_mvn_root_refine(const float* cov, const float* R, int B, int n, float jitter, float* ws,
                               float* Rout, hipStream_t stream) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_mvn_root_refine_kernel,
                              hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024);
    (void)hipGetLastError();
  });
  const int T = (n + 15) / 16;
  const size_t lds = ((size_t)(T * (T + 1) / 2) + (size_t)T) * 256 * sizeof(float);
  hipLaunchKernelGGL(gpk_mvn_root_refine_kernel, dim3((unsigned)B), dim3(256), lds, stream, cov, R, B, n, jitter,
                     ws, Rout);
  return (int)hipGetLastError();
}
