// Appending observations to a cached exact-GP factor (gpk_exact_append_f32) for gfx950.
//
// Replaces, per window b, what upstream models/exact_gp.py get_fantasy_model reaches through
// exact_prediction_strategies.py get_fantasy_strategy: the factor and the whitened targets of the
// training data with m new points (Xn, yn) appended, from the cached L and z = L^{-1}(y - c):
//   V  = L^{-1} K(X, Xn)                        phase 1 of the joint posterior (stored V)
//   S  = K(Xn, Xn) + (noise + jitter) I - V^T V  its phase 2, the noise added here
//   R  = chol(S)                                gpk_mvn_root's factorisation
//   zn = R^{-1} (yn - c - V^T z)                gpk_tri_solve against R
//   L' = [[L, 0], [V^T, R]]     z' = [z ; zn]   the finish kernel below
// By the uniqueness of the Cholesky factor L', z' are what gpk_exact_mll_f32 returns for the
// concatenated data (up to rounding), in its layout: the full square, upper triangle zero.
//
// New device code, both memory-bound:
//   prep:   S_ii += hyp[1] of the window's own hyper row, d = yn - mean (one thread per new point);
//   finish: the (B, N', N') output, N' = N + m. A window's work is cut into items, dealt round
//     robin to the G workgroups of the window (G grows as B shrinks, so a few windows still fill
//     the device):
//       - 16 rows of L -> Lout with the m zeros behind each: one wave per row, 16-byte stores from
//         the row's first 16-byte boundary on (N' is arbitrary: a scalar head and tail), 16-byte
//         loads when the source is aligned at that point too, four dword loads otherwise;
//       - a 64 x 64 tile of V -> V^T in rows N..: read along V's vs-strided rows, written along
//         Lout's rows, transposed through LDS (row stride 65: no bank conflict either way);
//       - 16 rows of R into the corner; z and zn into zout.
//     A window whose Schur complement did not factor (info != 0) gets NaN in R's block and in zn.
// Bit-exact copies, no atomics, fixed order everywhere: a second call gives the same bits.
#include "gpk_common.h"
#include "gpk_posterior_cov.h"

namespace {

constexpr int kApRows = 16;   // rows of L (or of R) per item
constexpr int kApT = 64;      // edge of a transposed tile of V
constexpr int kApWgs = 2048;  // workgroups a launch aims for: 8 per CU

struct GpkAppendFinishArgs {
  const float* L;      // (B, N, N)
  const float* z;      // (B, N)
  const float* V;      // (B, N, vs)
  const float* R;      // (B, m, m), upper triangle zero
  const float* zn;     // (B, m)
  const int* info;     // (B,)
  int B, N, m, vs, G;
  float* Lout;         // (B, N + m, N + m)
  float* zout;         // (B, N + m)
};

__global__ __launch_bounds__(256) void gpk_append_prep_kernel(const float* __restrict__ hyp, long long hyp_stride,
                                                              const float* __restrict__ yn,
                                                              const float* __restrict__ mean, int B, int m,
                                                              float* __restrict__ S, float* __restrict__ d) {
  const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
  if (idx >= (long long)B * m) return;
  const long long b = idx / m;
  const int i = (int)(idx - b * m);
  S[((size_t)b * m + i) * m + i] += hyp[b * hyp_stride + 1];
  d[idx] = yn[idx] - mean[idx];
}

// dst[0 .. n) = src[0 .. ns) followed by zeros, by one wave.
GPK_DEVICE void ap_row(float* __restrict__ dst, const float* __restrict__ src, int ns, int n, int lane) {
  int head = (int)(((16 - ((uintptr_t)dst & 15)) & 15) >> 2);
  if (head > n) head = n;
  if (lane < head) dst[lane] = lane < ns ? src[lane] : 0.f;
  const int nv = (n - head) >> 2;
  const bool src_al = ((uintptr_t)(src + head) & 15) == 0;
  for (int q = lane; q < nv; q += 64) {
    const int j = head + 4 * q;
    f32x4 v;
    if (src_al && j + 4 <= ns) {
      v = *(const f32x4*)&src[j];
    } else {
#pragma unroll
      for (int t = 0; t < 4; ++t) v[t] = j + t < ns ? src[j + t] : 0.f;
    }
    *(f32x4*)&dst[j] = v;
  }
  const int j = head + 4 * nv + lane;
  if (lane < 4 && j < n) dst[j] = j < ns ? src[j] : 0.f;
}

__global__ __launch_bounds__(256) void gpk_append_finish_kernel(GpkAppendFinishArgs a) {
  __shared__ float tile[kApT * (kApT + 1)];
  const int tid = threadIdx.x, lane = tid & 63;
  const int w = wave_id_uniform();
  const int b = blockIdx.x / a.G, g = blockIdx.x - b * a.G;
  const int N = a.N, m = a.m, Np = N + m, vs = a.vs;
  const int nA = (N + kApRows - 1) / kApRows;
  const int tk = (N + kApT - 1) / kApT, nB = tk * ((m + kApT - 1) / kApT);
  const int nC = (m + kApRows - 1) / kApRows;
  const int total = nA + nB + nC + 1;
  const float* Lb = a.L + (size_t)b * N * N;
  const float* Vb = a.V + (size_t)b * N * vs;
  const float* Rb = a.R + (size_t)b * m * m;
  float* Lo = a.Lout + (size_t)b * Np * Np;
  const bool ok = a.info[b] == 0;
  const float nan = __builtin_nanf("");

  for (int it = g; it < total; it += a.G) {   // the same items for every thread of the workgroup
    if (it < nA) {
      const int r1 = kApRows * it + kApRows < N ? kApRows * it + kApRows : N;
      for (int r = kApRows * it + w; r < r1; r += 4) ap_row(Lo + (size_t)r * Np, Lb + (size_t)r * N, N, Np, lane);
    } else if (it < nA + nB) {
      const int t = it - nA, ci = t / tk, ki = t - ci * tk;
      const int c0 = kApT * ci, k0 = kApT * ki;
      lds_barrier();   // the previous tile's reads are done
      for (int e = tid; e < kApT * kApT; e += 256) {
        const int kr = e >> 6, c = e & 63;
        tile[kr * (kApT + 1) + c] = (k0 + kr < N && c0 + c < m) ? Vb[(size_t)(k0 + kr) * vs + c0 + c] : 0.f;
      }
      lds_barrier();
      for (int e = tid; e < kApT * kApT; e += 256) {
        const int c = e >> 6, kr = e & 63;
        if (c0 + c < m && k0 + kr < N) Lo[(size_t)(N + c0 + c) * Np + k0 + kr] = tile[kr * (kApT + 1) + c];
      }
    } else if (it < nA + nB + nC) {
      const int i0 = kApRows * (it - nA - nB);
      for (int e = tid; e < kApRows * m; e += 256) {
        const int i = i0 + e / m, j = e % m;
        if (i < m) Lo[(size_t)(N + i) * Np + N + j] = ok ? Rb[(size_t)i * m + j] : nan;
      }
    } else {
      const float* zb = a.z + (size_t)b * N;
      const float* znb = a.zn + (size_t)b * m;
      float* zo = a.zout + (size_t)b * Np;
      for (int i = tid; i < Np; i += 256) zo[i] = i < N ? zb[i] : (ok ? znb[i - N] : nan);
    }
  }
}

}  // namespace

// Floats of workspace behind phase 1's V and training mean (gpk_post_cov_ws_floats(B, N, m)):
// S and R (B, m, m each), then the posterior mean and variance at Xn, d = yn - mean and zn (B, m each).
size_t gpk_exact_append_ws_floats(int B, int N, int m) {
  return gpk_post_cov_ws_floats(B, N, m) + (size_t)B * (2 * (size_t)m * m + 4 * (size_t)m);
}

int gpk_launch_exact_append(const float* X, const float* L, const float* z, const float* hyp, int n_ls,
                            long long hyp_stride, const float* Xn, const float* yn, int B, int N, int m, int D,
                            float jitter, float* ws, float* Lout, float* zout, int* info, hipStream_t stream) {
  const int vs = gpk_post_cov_vstride(m);
  float* V = ws;
  float* mu = V + (size_t)B * N * vs;
  float* S = ws + gpk_post_cov_ws_floats(B, N, m);
  float* R = S + (size_t)B * m * m;
  float* mean = R + (size_t)B * m * m;
  float* var = mean + (size_t)B * m;
  float* d = var + (size_t)B * m;
  float* zn = d + (size_t)B * m;

  GpkPostVArgs p{};
  static_cast<GpkPostArgs&>(p) = GpkPostArgs{X, L, z, hyp, n_ls, Xn, B, N, m, D, mean, var, hyp_stride};
  p.V = V;
  p.mu = mu;
  p.vs = vs;
  int rc = N > kGpkExactRegMaxN ? gpk_launch_exact_large_posterior_storev(p, stream)
                                : gpk_launch_exact_posterior_storev(p, stream);
  if (rc != 0) return rc;
  GpkPostCovArgs c{hyp, n_ls, Xn, V, mu, var, B, N, m, D, vs, S, hyp_stride};
  rc = gpk_launch_exact_posterior_cov(c, stream);
  if (rc != 0) return rc;

  const long long pts = (long long)B * m;
  hipLaunchKernelGGL(gpk_append_prep_kernel, dim3((unsigned)((pts + 255) / 256)), dim3(256), 0, stream, hyp,
                     hyp_stride, yn, mean, B, m, S, d);
  rc = (int)hipGetLastError();
  if (rc != 0) return rc;
  rc = gpk_launch_mvn_root(S, nullptr, nullptr, B, m, 0, jitter, R, nullptr, info, stream);
  if (rc != 0) return rc;
  rc = gpk_launch_tri_solve(R, d, B, m, 0, zn, stream);
  if (rc != 0) return rc;

  const int items = (N + kApRows - 1) / kApRows + ((N + kApT - 1) / kApT) * ((m + kApT - 1) / kApT) +
                    (m + kApRows - 1) / kApRows + 1;
  int G = (kApWgs + B - 1) / B;
  if (G > items) G = items;
  if ((long long)B * G > 0x7fffffff) return -8;
  GpkAppendFinishArgs f{L, z, V, R, zn, info, B, N, m, vs, G, Lout, zout};
  hipLaunchKernelGGL(gpk_append_finish_kernel, dim3((unsigned)(B * G)), dim3(256), 0, stream, f);
  return (int)hipGetLastError();
}
