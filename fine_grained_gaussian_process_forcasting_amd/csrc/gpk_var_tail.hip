// Variational hot path, the tail every path shares: gpk_var_ell_kernel after a forward;
// gpk_dlinv_kernel (paths with a dA / K_ZX workspace), gpk_var_red_kernel and gpk_var_fin_kernel
// after an adjoint.
//   gpk_var_ell_kernel  per-window ELL sum from the written mean / var (fixed order: deterministic).
//   gpk_dlinv_kernel    dL^{-1} = sum_points dA K_ZX^T: split-K fp64-MFMA GEMM, 64 x 64 lower tiles;
//   gpk_var_red_kernel / gpk_var_fin_kernel  fixed-order sums of the partials -> outputs.
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

namespace {

// Per-window ELL sum (fixed summation order: run-to-run deterministic).
__global__ void __launch_bounds__(256)
gpk_var_ell_kernel(const float* __restrict__ mean, const float* __restrict__ var,
                   const float* __restrict__ y, const float* __restrict__ hyp, int N,
                   float* __restrict__ ell) {
  __shared__ float red[4];
  const int b = blockIdx.x, tid = threadIdx.x;
  const float noise = hyp[1];
  const float log_noise = __logf(noise);
  float acc = 0.f;
  for (int i = tid; i < N; i += 256) {
    const size_t o = (size_t)b * N + i;
    const float dy = y[o] - mean[o];
    acc += -0.5f * ((dy * dy + var[o]) / noise + log_noise + kLog2PiF);
  }
  acc = wave_sum(acc);
  if ((tid & 63) == 0) red[tid >> 6] = acc;
  lds_barrier();
  if (tid == 0) ell[b] = (red[0] + red[1]) + (red[2] + red[3]);
}

// dL^{-1}[p][q] = m_p u_q + 2 (s_p^2 - 1) G'[p][q] for q <= p, 0 above (fp64), elementwise from
// the fixed-order totals gtot (G' lower tiles in acc layout | u).
GPK_DEVICE void var_gdl_elem(long long e, const double* __restrict__ gtot, const float* __restrict__ vmean,
                             const float* __restrict__ vstd, int M, int MB, double* __restrict__ dLinv) {
  if (e >= (long long)M * M) return;
  const int p = (int)(e / M), q = (int)(e - (long long)p * M);
  double v = 0.0;
  if (q <= p) {
    const int ti = p >> 4, tj = q >> 4, ra = p & 15, cb = q & 15;
    const double gp = gtot[(ti * (ti + 1) / 2 + tj) * 256 + ((ra >> 2) * 16 + cb) * 4 + (ra & 3)];
    const double u = gtot[(size_t)(MB * (MB + 1) / 2) * 256 + q];
    const double sd = (double)vstd[p];
    v = (double)vmean[p] * u + 2.0 * (sd * sd - 1.0) * gp;
  }
  dLinv[e] = v;
}

// ---------------------------------------------------------------------------
// dL^{-1} = sum_cols dA[:, col] K[:, col]^T (lower part): split-K fp64-MFMA GEMM.
// Workgroup = one 64 x 64 lower output tile (ti >= tj) x one split of the columns;
// 4 waves, each a 32 x 32 quadrant (2 x 2 MFMA tiles). fp32 operands are exact in fp64.
// Partials -> ws (split, tile, 64 x 64) doubles.
// ---------------------------------------------------------------------------
constexpr int DLST = 34;   // LDS row stride (floats): 2c + g spreads the MFMA operand reads

__global__ void __launch_bounds__(256)
gpk_dlinv_kernel(const float* __restrict__ dA, const float* __restrict__ Kz, int M, long long BN,
                 int ntiles, long long cols_per_split, double* __restrict__ part, GpkOStr bs) {
  GPK_O_ADD(dA, bs.ws);
  GPK_O_ADD(Kz, bs.ws);
  GPK_O_ADD(part, bs.ws / 2);
  __shared__ float sa[64 * DLST];
  __shared__ float sb[64 * DLST];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int wave = tid >> 6, qr = wave >> 1, qc = wave & 1;
  const int tile = blockIdx.x % ntiles, split = blockIdx.x / ntiles;
  int ti = 0;
  while ((ti + 1) * (ti + 2) / 2 <= tile) ++ti;
  const int tj = tile - ti * (ti + 1) / 2;
  const int m0 = 64 * ti, p0 = 64 * tj;
  const long long c0 = (long long)split * cols_per_split;
  long long c1 = c0 + cols_per_split;
  c1 = c1 < BN ? c1 : BN;
  const bool vec = (BN & 3) == 0;   // 16-B loads need 16-B aligned rows
  f64x4 acc[2][2];
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v) acc[u][v] = f64x4{0.0, 0.0, 0.0, 0.0};
  // each thread stages 2 x 4 consecutive columns of one row of each operand per step:
  // e = tid + 256 h (h = 0, 1) -> row e / 8, columns 4 (e % 8) .. +3
  float4 ra[2], rb[2];
  auto load = [&](long long cb, float4 (&xa)[2], float4 (&xb)[2]) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = tid + 256 * h, rr = e >> 3, k4 = 4 * (e & 7);
      const long long col = cb + k4;
      float4 va = {0.f, 0.f, 0.f, 0.f}, vb = {0.f, 0.f, 0.f, 0.f};
      if (vec && col + 3 < c1) {
        if (m0 + rr < M) va = *(const float4*)&dA[(size_t)(m0 + rr) * BN + col];
        if (p0 + rr < M) vb = *(const float4*)&Kz[(size_t)(p0 + rr) * BN + col];
      } else {
        float ta[4], tb[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool ok = col + u < c1;
          ta[u] = (ok && m0 + rr < M) ? dA[(size_t)(m0 + rr) * BN + col + u] : 0.f;
          tb[u] = (ok && p0 + rr < M) ? Kz[(size_t)(p0 + rr) * BN + col + u] : 0.f;
        }
        va = float4{ta[0], ta[1], ta[2], ta[3]};
        vb = float4{tb[0], tb[1], tb[2], tb[3]};
      }
      xa[h] = va;
      xb[h] = vb;
    }
  };
  load(c0, ra, rb);
  for (long long cb = c0; cb < c1; cb += DLKC) {
    lds_barrier();  // previous step's MFMA operand reads are done
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int e = tid + 256 * h, rr = e >> 3, k4 = 4 * (e & 7);
      *(float2*)&sa[rr * DLST + k4] = float2{ra[h].x, ra[h].y};
      *(float2*)&sa[rr * DLST + k4 + 2] = float2{ra[h].z, ra[h].w};
      *(float2*)&sb[rr * DLST + k4] = float2{rb[h].x, rb[h].y};
      *(float2*)&sb[rr * DLST + k4 + 2] = float2{rb[h].z, rb[h].w};
    }
    lds_barrier();
    if (cb + DLKC < c1) load(cb + DLKC, ra, rb);   // next step's loads overlap the MFMAs
#pragma unroll
    for (int k = 0; k < DLKC / 4; ++k) {
      double a[2], bb[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        a[u] = (double)sa[(32 * qr + 16 * u + c) * DLST + 4 * k + g];
        bb[u] = (double)sb[(32 * qc + 16 * u + c) * DLST + 4 * k + g];
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
#pragma unroll
        for (int v = 0; v < 2; ++v) acc[u][v] = mfma64(a[u], bb[v], acc[u][v]);
    }
  }
  double* po = part + ((size_t)split * ntiles + tile) * 4096;
#pragma unroll
  for (int u = 0; u < 2; ++u)
#pragma unroll
    for (int v = 0; v < 2; ++v)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = 32 * qr + 16 * u + g + 4 * r, col = 32 * qc + 16 * v + c;
        po[row * 64 + col] = acc[u][v][r];
      }
}

// Fixed-order reductions, 32 outputs per workgroup, 8 lanes per output each summing
// every 8th partial, then the 8 lane sums in a fixed order (fp64):
//   (a) the per-workgroup adjoint partials -> tot (P doubles);
//   (b) the split-K dL^{-1} partials -> dLinv (M x M, upper zero).
__global__ void __launch_bounds__(256)
gpk_var_red_kernel(const float* __restrict__ wspart, int nwg, int P, double* __restrict__ tot,
                   const double* __restrict__ dlpart, int nsplit, int ntiles, int M,
                   double* __restrict__ dLinv, const float* __restrict__ wspart2, int P2,
                   double* __restrict__ tot2, GpkOStr bs) {
  GPK_O_ADD(wspart, bs.ws);
  GPK_O_ADD(tot, bs.ws / 2);
  GPK_O_OPT(dlpart, bs.ws / 2);
  GPK_O_OPT(dLinv, M * M);
  GPK_O_OPT(wspart2, bs.ws);
  GPK_O_OPT(tot2, bs.ws / 2);
  __shared__ double red[8][33];
  const int tid = threadIdx.x, o = tid & 31, q0 = tid >> 5;
  const int nblk_a = (P + 31) / 32;
  double s = 0.0;
  long long out;
  if ((int)blockIdx.x < nblk_a) {
    out = (long long)blockIdx.x * 32 + o;
    if (out < P) {
#pragma unroll 4
      for (int q = q0; q < nwg; q += 8) s += (double)wspart[(size_t)q * P + out];
    }
  } else if (wspart2 != nullptr) {
    // a second partial array with the same workgroup count (one launch for both sums)
    out = (long long)(blockIdx.x - nblk_a) * 32 + o;
    if (out < P2) {
#pragma unroll 4
      for (int q = q0; q < nwg; q += 8) s += (double)wspart2[(size_t)q * P2 + out];
    }
  } else {
    out = (long long)(blockIdx.x - nblk_a) * 32 + o;
    if (out < (long long)M * M) {
      const int m = (int)(out / M), p = (int)(out - (long long)m * M);
      if (p <= m) {
        const int ti = m >> 6, tj = p >> 6;
        const int tile = ti * (ti + 1) / 2 + tj;
        const int off = (m & 63) * 64 + (p & 63);
#pragma unroll 4
        for (int q = q0; q < nsplit; q += 8) s += dlpart[((size_t)q * ntiles + tile) * 4096 + off];
      }
    }
  }
  red[q0][o] = s;
  lds_barrier();
  if (q0 == 0) {
    double t = 0.0;
#pragma unroll
    for (int q = 0; q < 8; ++q) t += red[q][o];
    if ((int)blockIdx.x < nblk_a) {
      if (out < P) tot[out] = t;
    } else if (wspart2 != nullptr) {
      if (out < P2) tot2[out] = t;
    } else if (out < (long long)M * M) {
      dLinv[out] = t;
    }
  }
}

// Outputs from the reduced totals, ONE launch (gpk_var_fin_kernel):
//   blocks 0 .. nblk-1 (16 inducing points each):  dZ_p = (QX_p - zs_p q_p) / l
//   block nblk (the totals block, all M rows):
//       dl_d = (sum_p (q_p zs_pd^2 - 2 zs_pd QX_pd) + sum_i r_i xs_id^2) / l_d
//       ds2 = sum Q / s2 + sum gvar;    dvmean = sum gmean A;   dvstd = 2 s sum gvar A^2
//       dw_d = l_d (sum_i gmean_i xs_id + cm_d sum_i gmean_i);   db0 = sum_i gmean_i
//   block nblk + 1 (gd.gtot != nullptr, register path): dL^{-1} from the K-Gram totals
// dpar = [dvmean (M) | dvstd (M) | ds2 | dl (D) | dw (D) | db0]. zs = Z / l - cm with the centre
// cm from the adjoint kernel (cm_in: its stage_inducing) or, without it, recomputed by
// col_means -- the same fixed-order fp32 sums, so the identical centre. No block depends on
// another: the round-4 second launch (block partials of dl) is gone.
constexpr int kFinRows = 16;

GPK_DEVICE void var_gdl_block(const double* __restrict__ gtot, const double* __restrict__ Linv,
                              const float* __restrict__ vmean, const float* __restrict__ vstd, int M,
                              double* __restrict__ dLinv, double (*Gs)[65], double* us);

// gd.gtot != nullptr: dL^{-1} from the K-Gram totals in extra workgroups of the output launch
// instead of a launch of its own -- MB == 0 (register path, M <= 64): one workgroup
// (var_gdl_block, L^{-1} G on fp64 MFMA); MB > 0 (saved-state path): M^2 / 256 workgroups of
// the elementwise m u^T + 2 (s^2 - 1) G' (var_gdl_elem)
struct VarGdlArgs {
  const double* gtot;
  const double* Linv;
  const float* vmean;
  const float* vstd;
  double* dLinv;
  int MB;
};
GPK_DEVICE void var_gdl_elem(long long e, const double* __restrict__ gtot, const float* __restrict__ vmean,
                             const float* __restrict__ vstd, int M, int MB, double* __restrict__ dLinv);

__global__ void __launch_bounds__(256)
gpk_var_fin_kernel(const float* __restrict__ Z, const float* __restrict__ vstd,
                   const float* __restrict__ hyp, const double* __restrict__ tot, int M, int D,
                   float* __restrict__ dZ, float* __restrict__ dpar, const float* __restrict__ cm_in,
                   VarGdlArgs gd, GpkOStr bs) {
  GPK_O_ADD(Z, M * D);
  GPK_O_ADD(vstd, M);
  GPK_O_ADD(hyp, 4 + 2 * D);
  GPK_O_ADD(tot, bs.ws / 2);
  GPK_O_ADD(dZ, M * D);
  GPK_O_ADD(dpar, 2 * M + 2 * D + 2);
  GPK_O_OPT(cm_in, bs.ws);
  if (gd.gtot != nullptr) {
    GPK_O_ADD(gd.gtot, bs.ws / 2);
    GPK_O_ADD(gd.Linv, M * M);
    GPK_O_ADD(gd.vmean, M);
    GPK_O_ADD(gd.vstd, M);
    GPK_O_ADD(gd.dLinv, M * M);
  }
  extern __shared__ __attribute__((aligned(16))) float fzs[];   // M x D zs (centred Z / l)
  __shared__ double red[256];
  __shared__ float cmf[64];
  __shared__ float cms[kCmParts * 64];
  const int tid = threadIdx.x;
  const int nblk = (M + kFinRows - 1) / kFinRows;
  if (gd.gtot != nullptr && (int)blockIdx.x > nblk) {
    if (gd.MB == 0) {
      double* gl = (double*)fzs;
      var_gdl_block(gd.gtot, gd.Linv, gd.vmean, gd.vstd, M, gd.dLinv, (double(*)[65])gl, gl + 64 * 65);
    } else {
      var_gdl_elem((long long)(blockIdx.x - nblk - 1) * 256 + tid, gd.gtot, gd.vmean, gd.vstd, M, gd.MB,
                   gd.dLinv);
    }
    return;
  }
  const bool totals = (int)blockIdx.x == nblk;
  const float* ls = hyp + 4 + D;
  const int p0 = totals ? 0 : blockIdx.x * kFinRows;
  const int np = totals ? M : (M - p0 < kFinRows ? M - p0 : kFinRows);
  if (cm_in != nullptr) {
    // the centre from the adjoint kernel, so only this block's rows of Z are staged
    if (tid < D) cmf[tid] = cm_in[tid];
    for (int base = 0; base < np * D; base += 8 * 256) {
      float zv[8], lv[8], cv[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + 256 * u + tid, ec = e < np * D ? e : 0, d = ec % D;
        zv[u] = Z[(size_t)p0 * D + ec];
        lv[u] = ls[d];
        cv[u] = cm_in[d];
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = base + 256 * u + tid;
        if (e < np * D) fzs[p0 * D + e] = zv[u] / lv[u] - cv[u];
      }
    }
  } else {
    for (int base = 0; base < M * D; base += 32 * 256) {
      float zv[32], lv[32];
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const int e = base + 256 * u + tid, ec = e < M * D ? e : 0;
        zv[u] = Z[ec];
        lv[u] = ls[ec % D];
      }
#pragma unroll
      for (int u = 0; u < 32; ++u) {
        const int e = base + 256 * u + tid;
        if (e < M * D) fzs[e] = zv[u] / lv[u];
      }
    }
    lds_barrier();
    col_means(fzs, M, D, D, D, cms, cmf);   // the same fp32 sums as stage_inducing: the identical centre
    for (int e = tid; e < np * D; e += 256) fzs[p0 * D + e] -= cmf[e % D];
  }
  lds_barrier();
  const double* QX = tot;
  const double* q = tot + (size_t)M * D;
  if (!totals) {
    const int e = tid;   // np * D <= 16 * 64 = 1024: up to 4 per thread, loads together
    double xv[4], qv[4];
    float lv[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ee = e + 256 * u, ok = ee < np * D;
      const int p = p0 + (ok ? ee / D : 0), d = ok ? ee % D : 0;
      xv[u] = QX[(size_t)p * D + d];
      qv[u] = q[p];
      lv[u] = ls[d];
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int ee = e + 256 * u;
      if (ee < np * D) {
        const int p = p0 + ee / D, d = ee % D;
        const double zsv = (double)fzs[p * D + d];
        dZ[(size_t)p * D + d] = (float)((xv[u] - zsv * qv[u]) / (double)lv[u]);
      }
    }
    return;
  }
  // ---- the totals block: dl over all M rows, threads (d, k), k = tid / D, rows k, k + nk, ..
  // (16 rows' loads in flight per thread, fixed order)
  const double* dvm = tot + (size_t)M * D + M;
  const double* dsm = dvm + M;
  const double* rx2 = dsm + M;
  const double* gx = rx2 + D + 2;
  const int nk = 256 / D;
  double acc = 0.0;
  if (tid < nk * D) {
    const int d = tid % D, k = tid / D;
    for (int base = k; base < M; base += 16 * nk) {
      double qv[16], xv[16];
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int pl = base + nk * u, pc = pl < M ? pl : 0;
        qv[u] = q[pc];
        xv[u] = QX[(size_t)pc * D + d];
      }
#pragma unroll
      for (int u = 0; u < 16; ++u) {
        const int pl = base + nk * u;
        if (pl < M) {
          const double zsv = (double)fzs[pl * D + d];
          acc += qv[u] * zsv * zsv - 2.0 * zsv * xv[u];
        }
      }
    }
  }
  red[tid] = acc;
  lds_barrier();
  const float s2 = hyp[0];
  if (tid < D) {
    double v = rx2[tid];
    for (int k = 0; k < nk; ++k) v += red[k * D + tid];
    const double sumgm = gx[D];
    dpar[2 * M + 1 + tid] = (float)(v / (double)ls[tid]);
    dpar[2 * M + 1 + D + tid] = (float)((double)ls[tid] * (gx[tid] + (double)cmf[tid] * sumgm));
  }
  for (int m = tid; m < M; m += 256) {
    dpar[m] = (float)dvm[m];
    dpar[M + m] = (float)(2.0 * (double)vstd[m] * dsm[m]);
  }
  if (tid == 0) {
    const double sumQ = rx2[D], sumgv = rx2[D + 1], sumgm = gx[D];
    dpar[2 * M] = (float)(sumQ / (double)s2 + sumgv);
    dpar[2 * M + 1 + 2 * D] = (float)sumgm;
  }
}

// the two output launches (ws: nblk x D doubles of dl partials, then D floats of the centre)
int launch_var_fin(const GpkVarAdjArgs& a, const double* tot, GpkOStr bs, hipStream_t stream,
                   const float* cm_in = nullptr, const VarGdlArgs* gd = nullptr);

// dL^{-1}[p][k] = vm_p u_k + 2 (s_p^2 - 1) (L^{-1} G)[p][k]  (k <= p < M; upper zero) from the
// reduced totals (fp64). One workgroup: G (symmetric, from its lower tiles) in LDS, wave w
// forms the 16-row block w of L^{-1} G on fp64 MFMA with its L^{-1} operands requested up
// front (the triangular k-range: jb <= w).
// (256 threads; Gs: 64 x 65 doubles, us: 64 doubles of LDS)
GPK_DEVICE void var_gdl_block(const double* __restrict__ gtot, const double* __restrict__ Linv,
                              const float* __restrict__ vmean, const float* __restrict__ vstd, int M,
                              double* __restrict__ dLinv, double (*Gs)[65], double* us) {
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4;
  const int w = tid >> 6;
  // the 10 tile elements of this thread requested together (acc order: tile, reg r, lane)
  double gv[kGTiles];
#pragma unroll
  for (int t2 = 0; t2 < kGTiles; ++t2) gv[t2] = gtot[t2 * 256 + tid];
  const double uv = gtot[kGTiles * 256 + (tid & 63)];
#pragma unroll
  for (int t2 = 0; t2 < kGTiles; ++t2) {
    constexpr int kRt[kGTiles] = {0, 1, 1, 2, 2, 2, 3, 3, 3, 3};
    const int rt = kRt[t2], rp = t2 - rt * (rt + 1) / 2;
    const int r = tid >> 6, ln = tid & 63;
    const int row = 16 * rt + 4 * (ln >> 4) + r, col = 16 * rp + (ln & 15);   // f32 acc: row 4g + r
    if (rt == rp && row < col) continue;   // one writer per element: deterministic
    Gs[row][col] = gv[t2];
    Gs[col][row] = gv[t2];
  }
  if (tid < 64) us[tid] = uv;
  // A operands L^{-1}[16 w + c][16 jb + 4 s + g] for jb <= w, requested before the barrier
  double la[4][4];
#pragma unroll
  for (int jb = 0; jb < 4; ++jb)
#pragma unroll
    for (int s4 = 0; s4 < 4; ++s4) {
      const int p = 16 * w + c, j = 16 * jb + 4 * s4 + g;
      const bool ok = jb <= w && p < M && j < M;
      const double v = Linv[ok ? (size_t)p * M + j : 0];
      la[jb][s4] = ok ? v : 0.0;
    }
  lds_barrier();
#pragma unroll
  for (int kb = 0; kb < 4; ++kb) {
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int jb = 0; jb < 4; ++jb)
#pragma unroll
      for (int s4 = 0; s4 < 4; ++s4) acc = mfma64(la[jb][s4], Gs[16 * jb + 4 * s4 + g][16 * kb + c], acc);
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int p = 16 * w + g + 4 * r, k = 16 * kb + c;
      if (p < M && k < M) {
        const double sd = (double)vstd[p];
        dLinv[(size_t)p * M + k] = k <= p ? (double)vmean[p] * us[k] + 2.0 * (sd * sd - 1.0) * acc[r] : 0.0;
      }
    }
  }
}

int launch_var_fin(const GpkVarAdjArgs& a, const double* tot, GpkOStr bs, hipStream_t stream,
                   const float* cm_in, const VarGdlArgs* gd) {
  const int M = a.M, D = a.D;
  const int nblk = (M + kFinRows - 1) / kFinRows;
  set_lds_once<gpk_var_fin_kernel, 64 * 1024>();   // + ~3.3 KB static
  size_t lds = (size_t)M * D * sizeof(float);
  VarGdlArgs g{};
  int ngd = 0;
  if (gd != nullptr) {
    g = *gd;
    if (g.MB == 0) {
      ngd = 1;
      const size_t gl = (64 * 65 + 64) * sizeof(double);
      if (lds < gl) lds = gl;
    } else {
      ngd = (int)(((long long)M * M + 255) / 256);
    }
  }
  hipLaunchKernelGGL(gpk_var_fin_kernel, dim3(nblk + 1 + ngd, a.O), dim3(256), lds, stream, a.Z,
                     a.vstd, a.hyp, tot, M, D, a.dZ, a.dpar, cm_in, g, bs);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

}  // namespace

// dL^{-1} GEMM, the fixed-order reductions and the outputs (both adjoint paths)
int gpk_launch_var_adj_tail(const GpkVarAdjArgs& a, const AdjPlan& p, hipStream_t stream) {
  char* ws = (char*)a.ws;
  float* wsdA = (float*)(ws + p.off_dA);
  float* wsK = (float*)(ws + p.off_K);
  float* wspart = (float*)(ws + p.off_part);
  double* tot = (double*)(ws + p.off_tot);
  double* dl = (double*)(ws + p.off_dl);
  const GpkOStr bs = adj_strides(a, p.total);
  hipLaunchKernelGGL(gpk_dlinv_kernel, dim3(p.ntiles * p.nsplit, a.O), dim3(256), 0, stream, wsdA, wsK,
                     a.M, p.BN, p.ntiles, p.cols_per_split, dl, bs);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  const long long nred = (p.P + 31) / 32 + ((long long)a.M * a.M + 31) / 32;
  hipLaunchKernelGGL(gpk_var_red_kernel, dim3((unsigned)nred, a.O), dim3(256), 0, stream,
                     wspart, p.nwg, p.P, tot, dl, p.nsplit, p.ntiles, a.M, a.dLinv, nullptr, 0, nullptr, bs);
  e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return launch_var_fin(a, tot, bs, stream);
}

int gpk_launch_var_red(const GpkVarAdjArgs& a, hipStream_t stream, const float* wspart, int nwg, int P,
                       double* tot, const float* wspart2, int P2, double* tot2, GpkOStr bs) {
  const int nblk = (P + 31) / 32 + (wspart2 != nullptr ? (P2 + 31) / 32 : 0);
  hipLaunchKernelGGL(gpk_var_red_kernel, dim3(nblk, a.O), dim3(256), 0, stream, wspart, nwg, P, tot,
                     nullptr, 0, 0, 0, nullptr, wspart2, P2, tot2, bs);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}

int gpk_launch_var_fin(const GpkVarAdjArgs& a, const double* tot, GpkOStr bs, hipStream_t stream,
                       const float* cm_in, const double* gtot, int gdl_mb) {
  if (gtot == nullptr) return launch_var_fin(a, tot, bs, stream, cm_in);
  const VarGdlArgs gd{gtot, a.Linv, a.vmean, a.vstd, a.dLinv, gdl_mb};
  return launch_var_fin(a, tot, bs, stream, cm_in, &gd);
}

int gpk_launch_var_ell(const GpkVarArgs& a, hipStream_t stream) {
  hipLaunchKernelGGL(gpk_var_ell_kernel, dim3(a.B), dim3(256), 0, stream, a.mean, a.var, a.y,
                     a.hyp, a.N, a.ell);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? 0 : (int)e;
}
