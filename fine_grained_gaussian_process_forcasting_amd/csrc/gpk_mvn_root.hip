// Batched Cholesky root of dense covariances fused with sampling, for gfx950.
//
// Replaces upstream linear_operator utils/cholesky.py psd_safe_cholesky's
// torch.linalg.cholesky_ex (one rung of its jitter ladder: the host relaunches the whole batch
// with the next jitter, as upstream adds it to the whole batch) and MultivariateNormal.rsample's
// mean + R eps matmul (reference denoising_model/DeepGP.py:62-64 ``x.rsample()``).
//
// Design: one workgroup of 4 waves per matrix. The lower triangle lives in LDS as packed
// 16 x 16 tiles, T (T + 1) / 2 KB with T = ceil(n / 16) (dynamic LDS sized by n: several small
// matrices share a CU); n is padded to 16 T with an identity diagonal that is never stored.
// A tile holds the TRANSPOSE of its block in acc layout (gpk_common.h), element (row, col) of
// the block at float 4 (16 (col / 4) + row) + col % 4, so that for stored tiles Q, P
// mma_tn(Q, P) = block_Q block_P^T transposed: the panel and trailing products need no
// transposes and every operand is one ds_read_b128 per lane.
// Right-looking, 16 columns per step k:
//   1. wave 0 factors the diagonal tile (column by column, fixed order) and forms the inverse
//      of the 16 x 16 factor by forward substitution (lane c owns column c);
//   2. panel tile i > k:   P_i <- P_i inv^T           (mfma_f32_16x16x4f32, tiles over the waves)
//   3. trailing tile i >= j > k:  S_ij <- S_ij - P_i P_j^T   (same MFMA, tiles over the waves)
// A pivot that is not positive (or is NaN) sets an LDS flag; every wave reads the flag after
// the step's barrier and all leave the loop together: no wave returns in front of a barrier.
// After the last step the same workgroup writes R (upper triangle zero) and computes
// samples[s, b, i] = mean[b, i] + sum_{j <= i} R[i][j] eps[s, b, j] in ascending j from the
// factor still in LDS. All arithmetic fp32, fixed order, no atomics: deterministic.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"

#include <mutex>

namespace {

GPK_DEVICE int rt_el(int row, int col) { return 4 * (16 * (col >> 2) + row) + (col & 3); }
GPK_DEVICE int rt_tile(int i, int j) { return (i * (i + 1) / 2 + j) * 256; }

__global__ __launch_bounds__(256) void gpk_mvn_root_kernel(const float* __restrict__ cov,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ eps, int B, int n, int S,
                                                           float jitter, float* __restrict__ R,
                                                           float* __restrict__ samples, int* __restrict__ info) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int T = (n + 15) >> 4, np = 16 * T;
  float* tiles = lds;
  float* invT = lds + (size_t)(T * (T + 1) / 2) * 256;   // inverse of the diagonal factor; later eps
  int* flag = (int*)(invT + 256);
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int c = lane & 15, g = lane >> 4;
  const size_t b = blockIdx.x;
  const float* A = cov + b * (size_t)n * n;

  // ---- lower triangle (+ jitter on the diagonal) into the packed tiles, identity padding
  if (tid == 0) *flag = 0;
  for (int e = tid; e < np * np; e += 256) {
    const int i = e / np, j = e - i * np;
    if ((j >> 4) > (i >> 4)) continue;
    float v;
    if (i < n && j < n) {
      v = i >= j ? A[(size_t)i * n + j] : A[(size_t)j * n + i];   // only the lower triangle is read
      if (i == j) v += jitter;
    } else {
      v = i == j ? 1.f : 0.f;
    }
    tiles[rt_tile(i >> 4, j >> 4) + rt_el(i & 15, j & 15)] = v;
  }

  int bad = 0;
  for (int k = 0; k < T; ++k) {
    lds_barrier();
    float* Dk = tiles + rt_tile(k, k);
    if (w == 0) {
      int fail = 0;
      for (int j = 0; j < 16; ++j) {
        const float d = readlane_f(Dk[rt_el(j, j)], 0);
        if (!(d > 0.f)) { fail = 16 * k + j + 1; break; }
        const float r = __builtin_sqrtf(d);
        if (lane < 16) {
          if (lane > j) Dk[rt_el(lane, j)] = Dk[rt_el(lane, j)] / r;
          else if (lane == j) Dk[rt_el(j, j)] = r;
        }
        wave_lds_sync();
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          const int e = lane + 64 * q, i = e >> 4, l = e & 15;
          if (l > j && i >= l)
            Dk[rt_el(i, l)] = __builtin_fmaf(-Dk[rt_el(i, j)], Dk[rt_el(l, j)], Dk[rt_el(i, l)]);
        }
        wave_lds_sync();
      }
      if (fail != 0) {
        if (lane == 0) *flag = fail;
      } else if (k + 1 < T) {
        // inverse of the factor tile: lane c solves column c by forward substitution
        float x[16];
#pragma unroll
        for (int i = 0; i < 16; ++i) {
          float s = i == c ? 1.f : 0.f;
#pragma unroll
          for (int j = 0; j < i; ++j) s = __builtin_fmaf(-Dk[rt_el(i, j)], x[j], s);
          x[i] = s / Dk[rt_el(i, i)];
        }
        const f32x4 o = pick_group4(x, g);
#pragma unroll
        for (int r = 0; r < 4; ++r) invT[rt_el(4 * g + r, c)] = o[r];
      }
    }
    lds_barrier();
    bad = __builtin_amdgcn_readfirstlane(*as_lds_flags(flag));
    if (bad != 0) break;   // the same word for every wave: all leave together
    // ---- panel: P_i <- P_i inv^T
    {
      const f32x4 q = *(const f32x4*)&invT[4 * lane];
      for (int i = k + 1 + w; i < T; i += 4) {
        float* Pi = tiles + rt_tile(i, k);
        const f32x4 p = *(const f32x4*)&Pi[4 * lane];
        *(f32x4*)&Pi[4 * lane] = mma_tn(q, p, f32x4{0.f, 0.f, 0.f, 0.f});
      }
    }
    lds_barrier();
    // ---- trailing update: S_ij <- S_ij - P_i P_j^T, tiles round-robin over the waves
    int cnt = 0;
    for (int i = k + 1; i < T; ++i) {
      const f32x4 p = *(const f32x4*)&tiles[rt_tile(i, k) + 4 * lane];
      for (int j = k + 1; j <= i; ++j, ++cnt) {
        if ((cnt & 3) != w) continue;
        const f32x4 q = *(const f32x4*)&tiles[rt_tile(j, k) + 4 * lane];
        float* Sij = tiles + rt_tile(i, j);
        *(f32x4*)&Sij[4 * lane] = mma_tn(-q, p, *(const f32x4*)&Sij[4 * lane]);
      }
    }
  }
  lds_barrier();
  if (tid == 0) info[b] = bad;
  if (bad != 0) return;   // after the last barrier

  if (R != nullptr) {
    float* Rb = R + b * (size_t)n * n;
    for (int e = tid; e < n * n; e += 256) {
      const int i = e / n, j = e - i * n;
      Rb[e] = j <= i ? tiles[rt_tile(i >> 4, j >> 4) + rt_el(i & 15, j & 15)] : 0.f;
    }
  }
  for (int s = 0; s < S; ++s) {
    const size_t base = ((size_t)s * B + b) * (size_t)n;
    lds_barrier();   // the previous sample's reads of the staged eps are done
    for (int i = tid; i < n; i += 256) invT[i] = eps[base + i];
    lds_barrier();
    for (int i = tid; i < n; i += 256) {
      float acc = 0.f;
      const int ti = i >> 4, ri = i & 15;
      for (int j = 0; j <= i; ++j)
        acc = __builtin_fmaf(tiles[rt_tile(ti, j >> 4) + rt_el(ri, j & 15)], invT[j], acc);
      samples[base + i] = mean[b * (size_t)n + i] + acc;
    }
  }
}

}  // namespace

int gpk_launch_mvn_root(const float* cov, const float* mean, const float* eps, int B, int n, int S,
                        float jitter, float* R, float* samples, int* info, hipStream_t stream) {
  static std::once_flag once;
  std::call_once(once, [] {
    (void)hipFuncSetAttribute((const void*)gpk_mvn_root_kernel, hipFuncAttributeMaxDynamicSharedMemorySize,
                              160 * 1024);
    (void)hipGetLastError();
  });
  const int T = (n + 15) / 16;
  const size_t lds = ((size_t)(T * (T + 1) / 2) * 256 + 256 + 4) * sizeof(float);
  hipLaunchKernelGGL(gpk_mvn_root_kernel, dim3((unsigned)B), dim3(256), lds, stream, cov, mean, eps, B, n, S,
                     jitter, R, samples, info);
  return (int)hipGetLastError();
}
