// Dropping the oldest observations from a cached exact-GP factor (gpk_exact_drop_f32) for gfx950.
//
// Upstream GPyTorch has no counterpart: this is the inverse of get_fantasy_strategy's low-rank
// update (gpk_exact_append.hip), for a model that keeps a fixed look-back on a stream. Per window,
// with the cached factor split at row m,
//   L = [[L11, 0], [L21, L22]]    z = L^{-1}(y - c) = [z1 ; z2]    n = N - m,
// the kept points' matrix is L22 L22^T + U U^T with U = L21 (n x m), so the wanted factor is the
// positive rank-m update L' = chol(L22 L22^T + U U^T). In rotation form, for column j and
// t = 0 .. m-1, the rotation in the plane (L_:j, U_:t) that zeroes U_jt is applied to every row
// below j; [L22 | U] Q = [L' | 0]. The same rotations applied to the pair (z2_j, z1_t) give
// z' = L'^{-1}(y[m:] - c): (z2^T | z1^T) is carried as one more row of [L22 | U]. Neither the
// inputs X, y nor the hyper-parameters enter, and no pivot can fail.
//
// One workgroup per window, one thread per row (row n is the z row), 16-column block steps:
//   - a thread holds its row of U (m values, zero-padded to the instantiation's M: a rotation
//     against a zero is exactly the identity) and its 16 entries of the current block column in
//     registers for the whole kernel; the next block column's entries are loaded one step ahead;
//   - the wave that owns the 16 diagonal rows of block k ("phase A") walks the 16 columns: the
//     pivot row's U is broadcast lane by lane, lane t takes rho_{t-1}^2 and rho_t^2 of the prefix
//     form rho_t^2 = L_jj^2 + sum_{s<=t} U_js^2, so the m square roots and divisions of a column
//     are one lane-parallel evaluation (cos_t = rho_{t-1} / rho_t, sin_t = U_jt / rho_t), not a
//     dependent chain; the pairs go to LDS and are applied to the wave's own rows below the pivot;
//   - behind ONE workgroup barrier per block every later wave applies the 16 m rotations to its
//     rows from LDS (a uniform-address read per pair), stores the finished block column (zeros
//     above the diagonal, so the full square is written) and the wave that owns block k + 1 runs
//     its phase A into the other LDS buffer while the rest still apply block k.
// Instantiations M = 1, 2, 4, 8, 16, 32 (63 ... 107 VGPRs, no spills, 256 B ... 8 KiB of LDS); 64
// columns of U do not fit beside the two block columns in the 128 VGPRs a 13-wave workgroup leaves
// a thread, so m > 32 runs as two exact updates, rank 32 and rank m - 32, the second in place on
// Lout (a thread reads and writes its own row only).
// Rows of L and of Lout start on a 16-byte boundary only when N (n) is a multiple of 4: every
// 16-byte access is taken only when the thread's own address is aligned, four dword accesses
// otherwise. No atomics, a fixed order, and a workgroup reads its own window only: two calls give
// the same bits, a permutation of the windows permutes the outputs, a NaN stays in its window.
#include "../../include/gpk.h"
#include "gpk_common.h"
#include "gpk_internal.h"

namespace {

constexpr int kDropMaxM = 64;       // gpk_exact_drop_max_m(): two passes of at most kDropPass
constexpr int kDropPass = 32;       // columns of U a thread holds in registers
constexpr int kDropCols = 16;       // columns per block step
constexpr int kDropThreads = 832;   // 13 waves: the 799 rows of n = 799 and the z row

// One rank-mu pass: the kept block A (n x n, lower), the mu columns U that leave, and the z row
// (zA | zU) beside them, each with its own row and window strides, so that a second pass reads
// the first one's output in place (a thread reads and writes its own row only).
struct GpkDropArgs {
  const float* A;    // row i of window b at A + b * A_win + i * lda
  const float* U;    // row i of window b at U + b * U_win + i * ldu, mu columns
  const float* zA;   // (n) of window b at zA + b * zA_win
  const float* zU;   // (mu) of window b at zU + b * zU_win
  long long A_win, U_win, zA_win, zU_win;
  int lda, ldu, mu, n;
  float* Lout;       // (B, n, n)
  float* zout;       // (B, n)
};

// The rotation (cos, sin) on the pair (l, u): l' = cos l + sin u, u' = cos u - sin l.
GPK_DEVICE void drop_rot(float c, float s, float& l, float& u) {
  const float ln = __builtin_fmaf(c, l, s * u);
  u = __builtin_fmaf(c, u, -(s * l));
  l = ln;
}

// v[0 .. 16) = src[j0 .. j0 + 16), zero from column `lim` on.
GPK_DEVICE void drop_load16(float (&v)[kDropCols], const float* src, bool al, int j0, int lim) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + 4 * q;
    if (al && j + 4 <= lim) {
      const f32x4 x = *(const f32x4*)&src[j];
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * q + r] = x[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r) v[4 * q + r] = j + r < lim ? src[j + r] : 0.f;
    }
  }
}

// dst[j0 .. min(j0 + 16, n)) = v.
GPK_DEVICE void drop_store16(float* dst, bool al, int j0, int n, const float (&v)[kDropCols]) {
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int j = j0 + 4 * q;
    if (al && j + 4 <= n) {
      *(f32x4*)&dst[j] = f32x4{v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]};
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (j + r < n) dst[j + r] = v[4 * q + r];
    }
  }
}

// Phase A of the block column at j0, by the wave that owns its diagonal rows (all 64 lanes).
template <int M>
GPK_DEVICE void drop_diag(float (&Lr)[kDropCols], float (&u)[M], int i, int lane, int j0, int nj,
                          float2* __restrict__ cs) {
#pragma unroll
  for (int jj = 0; jj < kDropCols; ++jj) {
    if (jj >= nj) continue;              // the tail block: wave-uniform
    const int p = (j0 + jj) & 63;        // the pivot row's lane
    const float a = readlane_f(Lr[jj], p);
    float r2 = a * a, bt = 0.f, r2p = 1.f;
#pragma unroll
    for (int t = 0; t < M; ++t) {
      const float b = readlane_f(u[t], p);
      if (lane == t) {
        bt = b;
        r2p = r2;
      }
      r2 = __builtin_fmaf(b, b, r2);
    }
    // lane t < M: rho_{t-1} (rho_{-1} = L_jj itself) and rho_t
    const float rc = __builtin_sqrtf(__builtin_fmaf(bt, bt, r2p));
    const float rp = lane == 0 ? a : __builtin_sqrtf(r2p);
    const float c = rp / rc, s = bt / rc;
    if (lane < M) cs[jj * M + lane] = make_float2(c, s);
    const float rho = readlane_f(rc, M - 1);
    const bool below = i > j0 + jj, pivot = i == j0 + jj;
    float l = Lr[jj];
#pragma unroll
    for (int t = 0; t < M; ++t) {
      float ln = l, un = u[t];
      drop_rot(readlane_f(c, t), readlane_f(s, t), ln, un);
      l = below ? ln : l;
      u[t] = below ? un : (pivot ? 0.f : u[t]);
    }
    Lr[jj] = pivot ? rho : l;
  }
}

template <int M>
__global__ __launch_bounds__(kDropThreads) void gpk_exact_drop_kernel(GpkDropArgs a) {
  __shared__ float2 cs[2 * kDropCols * M];   // (cos, sin) of a block column, double-buffered
  const int i = threadIdx.x, lane = i & 63;
  const int w = wave_id_uniform();
  const int m = a.mu, n = a.n;
  const size_t b = blockIdx.x;
  // row i < n: a row of [A | U]; row n: (zA^T | zU^T); rows above n idle (all zero)
  const bool zrow = i == n, live = i <= n;
  const size_t ir = live ? i : 0;
  const float* usrc = zrow ? a.zU + b * a.zU_win : a.U + b * a.U_win + ir * a.ldu;
  const float* lsrc = zrow ? a.zA + b * a.zA_win : a.A + b * a.A_win + ir * a.lda;
  float* dst = zrow ? a.zout + b * n : a.Lout + (b * n + ir) * n;
  const int lim = !live ? 0 : (zrow ? n : i + 1);   // columns this row holds: the lower triangle
  const int nst = live ? n : 0;                     // columns this row writes
  const bool al_u = ((uintptr_t)usrc & 15) == 0, al_l = ((uintptr_t)lsrc & 15) == 0;
  const bool al_d = ((uintptr_t)dst & 15) == 0;

  float u[M];
#pragma unroll
  for (int q = 0; q < (M + 3) / 4; ++q) {
    if (al_u && live && 4 * q + 4 <= m) {
      const f32x4 x = *(const f32x4*)&usrc[4 * q];
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * q + r < M) u[4 * q + r] = x[r];
    } else {
#pragma unroll
      for (int r = 0; r < 4; ++r)
        if (4 * q + r < M) u[4 * q + r] = (live && 4 * q + r < m) ? usrc[4 * q + r] : 0.f;
    }
  }
  float Lr[kDropCols], Ln[kDropCols];
  drop_load16(Lr, lsrc, al_l, 0, lim);

  const int nblk = (n + kDropCols - 1) / kDropCols;
  if (w == 0) drop_diag<M>(Lr, u, i, lane, 0, n < kDropCols ? n : kDropCols, cs);

  for (int k = 0; k < nblk; ++k) {
    const int j0 = kDropCols * k, nj = n - j0 < kDropCols ? n - j0 : kDropCols;
    const bool more = k + 1 < nblk;
    if (more) drop_load16(Ln, lsrc, al_l, j0 + kDropCols, lim);
    lds_barrier();   // block k's pairs are in cs[k & 1]; cs[(k + 1) & 1] is free
    if (w > (j0 >> 6)) {   // the diagonal wave applied them in its phase A; earlier waves are done
      const float2* ck = cs + (k & 1) * kDropCols * M;
#pragma unroll
      for (int jj = 0; jj < kDropCols; ++jj) {
        if (jj >= nj) continue;
        float l = Lr[jj];
#pragma unroll
        for (int t = 0; t < M; ++t) {
          const float2 p = ck[jj * M + t];
          drop_rot(p.x, p.y, l, u[t]);
        }
        Lr[jj] = l;
      }
    }
    drop_store16(dst, al_d, j0, nst, Lr);
    if (more) {
#pragma unroll
      for (int c = 0; c < kDropCols; ++c) Lr[c] = Ln[c];
      const int j1 = j0 + kDropCols;
      if (w == (j1 >> 6))
        drop_diag<M>(Lr, u, i, lane, j1, n - j1 < kDropCols ? n - j1 : kDropCols, cs + ((k + 1) & 1) * kDropCols * M);
    }
  }
}

template <int M>
int drop_launch(const GpkDropArgs& a, int B, hipStream_t stream) {
  const int threads = (a.n + 1 + 63) / 64 * 64;   // the n rows and the z row
  hipLaunchKernelGGL(gpk_exact_drop_kernel<M>, dim3((unsigned)B), dim3(threads), 0, stream, a);
  return (int)hipGetLastError();
}

int drop_pass(const GpkDropArgs& a, int B, hipStream_t s) {
  if (a.mu <= 1) return drop_launch<1>(a, B, s);
  if (a.mu <= 2) return drop_launch<2>(a, B, s);
  if (a.mu <= 4) return drop_launch<4>(a, B, s);
  if (a.mu <= 8) return drop_launch<8>(a, B, s);
  if (a.mu <= 16) return drop_launch<16>(a, B, s);
  return drop_launch<kDropPass>(a, B, s);
}

bool drop_overlap(const float* p, size_t np, const float* q, size_t nq) {
  const uintptr_t p0 = (uintptr_t)p, q0 = (uintptr_t)q;
  return p0 < q0 + nq * sizeof(float) && q0 < p0 + np * sizeof(float);
}

}  // namespace

extern "C" {

int gpk_exact_drop_max_m(void) { return kDropMaxM; }

int gpk_exact_drop_f32(const float* L, const float* z, int B, int N, int m, float* Lout, float* zout,
                       void* stream) {
  if (L == nullptr) return -1;
  if (z == nullptr) return -2;
  if (B < 0) return -3;
  if (N < 1 || N > kGpkExactMaxN) return -4;
  if (m < 1 || m > kDropMaxM || m >= N) return -5;
  if (Lout == nullptr) return -6;
  if (zout == nullptr) return -7;
  const int n = N - m;
  const size_t nL = (size_t)B * N * N, nz = (size_t)B * N, nLo = (size_t)B * n * n, nzo = (size_t)B * n;
  if (Lout == L || drop_overlap(Lout, nLo, L, nL) || drop_overlap(Lout, nLo, z, nz)) return -6;
  if (zout == z || drop_overlap(zout, nzo, L, nL) || drop_overlap(zout, nzo, z, nz) ||
      drop_overlap(zout, nzo, Lout, nLo))
    return -7;
  if (B == 0) return 0;
  hipStream_t s = (hipStream_t)stream;
  const long long NN = (long long)N * N, nn = (long long)n * n;
  const float* A = L + (size_t)m * N + m;
  const float* U = L + (size_t)m * N;
  if (m <= kDropPass) return drop_pass(GpkDropArgs{A, U, z + m, z, NN, NN, N, N, N, N, m, n, Lout, zout}, B, s);
  // a rank-m update is two exact rank-<=32 updates: L22 L22^T + U1 U1^T, then + U2 U2^T in place
  const int rc = drop_pass(GpkDropArgs{A, U, z + m, z, NN, NN, N, N, N, N, kDropPass, n, Lout, zout}, B, s);
  if (rc != 0) return rc;
  return drop_pass(GpkDropArgs{Lout, U + kDropPass, zout, z + kDropPass, nn, NN, n, N, n, N, m - kDropPass, n, Lout,
                               zout}, B, s);
}

}  // extern "C"
