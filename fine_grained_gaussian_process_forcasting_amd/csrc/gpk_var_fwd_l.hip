// Variational hot path, L^{-1}-in-registers forward: gpk_var_fwd_l_kernel. Shapes: M > 64
// (GPK_VAR_LREG), every D; the training forward keeps A (LSaved) where the saved-state adjoint
// serves the shape (var_saved_path).
#include "gpk_var_common.h"
#include "gpk_var_launch.h"

namespace {

// ---------------------------------------------------------------------------
// Forward for M > 64 (cfg-3 shape M = 256): L^{-1} held in REGISTERS for the whole launch.
// A persistent workgroup of NWV = ceil(MB/2) waves; wave w owns the row tiles rA = w and
// rB = MB-1-w, i.e. MB+1 16x16 blocks of the lower triangle of L^{-1} (the same count for
// every wave: balanced), loaded once as f64 MFMA A operands: slot s holds, on lane (c, g)
// at MFMA step u, L^{-1}[16 rt + c][16 kb + 4 g + u]. Per 32-point chunk:
//   stage   xs = x/l - mean(Z/l), |xs|^2 and x.w (16 threads per point, DPP row sums);
//   Gram    the K_ZX tiles of the wave's own row tiles on f32 MFMA -- the f32 C layout
//           (reg r <-> row 4g + r) IS the f64 B-operand layout of step u = r, so each tile is
//           one b128 LDS store, read back by every wave as one b128 per (kb, column tile);
//   GEMM    A[rt] += L^{-1}[rt, kb] K_ZX[kb] over the wave's MB+1 blocks (fp64 MFMA);
//   reduce  per-wave partials of sum_m A m and sum_m A^2 (s^2 - 1) -> LDS, one wave finishes
//           mean / variance while the others stage the next chunk (its points were loaded
//           into registers during this chunk's GEMM).
// The LDS-tiled kernel above re-read the L^{-1} triangle (272 KB) from L2 for every chunk.
// ---------------------------------------------------------------------------
template <int MB, int DQ>
__global__ void __launch_bounds__(64 * ((MB + 1) / 2), 2)
gpk_var_fwd_l_kernel(const float* __restrict__ X, const float* __restrict__ Z,
                     const double* __restrict__ Linv, const float* __restrict__ vmean,
                     const float* __restrict__ vstd, const float* __restrict__ hyp, int N, int M,
                     int D, int nchunks, float* __restrict__ mean_out, float* __restrict__ var_out,
                     int* __restrict__ flags, float* __restrict__ saved, GpkOStr bs) {
  GPK_O_MODEL();
  GPK_O_ADD(Linv, M * M);
  GPK_O_ADD(mean_out, bs.bn);
  GPK_O_ADD(var_out, bs.bn);
  GPK_O_OPT(saved, bs.sv);
  using G = LGeo<MB, DQ>;
  constexpr int NWV = G::NWV, NT = G::NT, DS = G::DS, NPASS = G::NPASS, DV = G::DV;
  extern __shared__ __attribute__((aligned(16))) float vsm[];
  const int tid = threadIdx.x, lane = tid & 63, c = lane & 15, g = lane >> 4, sub = tid & 15;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int rA = wave, rB = MB - 1 - wave;   // rB == rA: the middle wave of an odd MB
  // hyp: [s2, noise, jitter, b0, w[D], ls[D]]
  const float s2 = hyp[0], jit = hyp[2], b0 = hyp[3];
  const float* w = hyp + 4;
  const float* ls = hyp + 4 + D;
  const int nch = (N + LTW - 1) / LTW;

  // the wave's L^{-1} blocks -> registers. M % 16 == 0: two row bases, every slot one
  // 32-byte run at an immediate offset (no per-load address registers or masks -- with
  // them the 68 loads in flight at M = 256 overflowed the register file); otherwise
  // masked loads from clamped addresses, 4 slots in flight at a time.
  double Lr[MB + 1][4];
  if ((M & 15) == 0) {
    const double* baseA = Linv + (size_t)(16 * rA + c) * M + 4 * g;
    const double* baseB = Linv + (size_t)(16 * rB + c) * M + 4 * g - 16 * (rA + 1);
#pragma unroll
    for (int s = 0; s <= MB; ++s) {
      const bool isA = s <= rA;
      if (isA || rB != rA) {
        const double* src = (isA ? baseA : baseB) + 16 * s;
        const double2 v0 = *(const double2*)src, v1 = *(const double2*)(src + 2);
        Lr[s][0] = v0.x; Lr[s][1] = v0.y; Lr[s][2] = v1.x; Lr[s][3] = v1.y;
      } else {
#pragma unroll
        for (int u = 0; u < 4; ++u) Lr[s][u] = 0.0;
      }
    }
  } else {
#pragma unroll
    for (int s = 0; s <= MB; ++s) {
      const bool isA = s <= rA;
      const int rt = isA ? rA : rB, kb = isA ? s : s - rA - 1;
      const bool ok = isA || rB != rA;
      const int m = 16 * rt + c;
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int p = 16 * kb + 4 * g + u;
        const bool in = ok && m < M && p < M;
        const double v = Linv[in ? (size_t)m * M + p : 0];
        Lr[s][u] = in ? v : 0.0;
      }
      if ((s & 3) == 3) __builtin_amdgcn_sched_barrier(0);
    }
  }
  // per-thread staging constants: dims d = sub + 16 v
  float lsr[DV], wr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) {
    const int d = sub + 16 * v;
    lsr[v] = ls[d < D ? d : 0];
    wr[v] = d < D ? w[d] : 0.f;
  }
  float xr[NPASS][DV];
  auto load_x = [&](int t) {
    const int b = t / nch, i0 = (t - b * nch) * LTW;
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
      const int j = (tid >> 4) + q * (NT / 16), i = i0 + j;
      const bool ok = t < nchunks && j < LTW && i < N;
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const int d = sub + 16 * v;
        const bool okd = ok && d < D;
        const float x = X[okd ? ((size_t)b * N + i) * D + d : 0];
        xr[q][v] = okd ? x : 0.f;
      }
    }
  };
  load_x(blockIdx.x);
  stage_inducing(Z, ls, vmean, vstd, M, D, G::MP, DQ, DS, vsm + G::oZs, vsm + G::oZn, vsm + G::oCm,
                 vsm + G::oVm, vsm + G::oSm1, vsm + G::oKl);
  lds_barrier();
  float cmr[DV];
#pragma unroll
  for (int v = 0; v < DV; ++v) cmr[v] = vsm[G::oCm + sub + 16 * v];
  int clamped = 0, par = 0;

  for (int t = blockIdx.x; t < nchunks; t += gridDim.x, par ^= 1) {
    const int b = t / nch, i0 = (t - b * nch) * LTW;
    const int nvalid = N - i0 < LTW ? N - i0 : LTW;
    // every LDS address re-derived per chunk (hoisted, they pinned ~100 registers)
    float* sm = (float*)fresh_lds(vsm);
    float* Kl = sm + G::oKl;
    float* red = sm + G::oRed;
    const float* zs = sm + G::oZs;
    const float* zn = sm + G::oZn;
    const float* vm = sm + G::oVm;
    const float* sm1 = sm + G::oSm1;
    float* xs = sm + G::oXs;
    float* xn = sm + G::oXn;
    float* lin = sm + G::oLin + par * LTW;
    // stage the chunk's points (xs of the previous chunk was last read by its Gram, before
    // the previous GEMM barrier; lin is double-buffered against the finishing wave)
#pragma unroll
    for (int q = 0; q < NPASS; ++q) {
      const int j = (tid >> 4) + q * (NT / 16);
      float nrm = 0.f, lp = 0.f;
      const bool okj = j < nvalid;
#pragma unroll
      for (int v = 0; v < DV; ++v) {
        const int d = sub + 16 * v;
        const float xv = (okj && d < D) ? xr[q][v] / lsr[v] - cmr[v] : 0.f;
        nrm = __builtin_fmaf(xv, xv, nrm);
        lp = __builtin_fmaf(xr[q][v], wr[v], lp);
        if (j < LTW) xs[j * DS + d] = xv;
      }
      nrm = row16_sum_f(nrm);
      lp = row16_sum_f(lp);
      if (sub == 0 && j < LTW) {    // (row16_sum_f leaves the sum on all 16 lanes)
        xn[j] = nrm;
        lin[j] = lp;
      }
    }
    lds_barrier();
    // K_ZX tiles of the wave's row tiles
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int rt = h == 0 ? rA : rB;
      if (h == 1 && rB == rA) break;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        const float* za = zs + (16 * rt + c) * DS + g;
        const float* xb = xs + (16 * ct + c) * DS + g;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < DQ / 4; ++k) acc = mfma32(za[4 * k], xb[4 * k], acc);
        const int col = 16 * ct + c;
        const float xnc = xn[col];
        f32x4 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int p = 16 * rt + 4 * g + r;
          float dist = zn[p] + xnc - 2.f * acc[r];
          dist = dist < 0.f ? 0.f : dist;
          o[r] = (p < M && col < nvalid) ? s2 * __builtin_amdgcn_exp2f(kNHalfLog2e * dist) : 0.f;
        }
        *(f32x4*)(Kl + ((rt * 2 + ct) * 64 + lane) * 4) = o;
      }
    }
    if (t + (int)gridDim.x < nchunks) load_x(t + gridDim.x);   // next chunk's points
    lds_barrier();
    // A = L^{-1} K_ZX on the wave's row tiles (code specialised per wave: the slot -> row
    // tile switch at rA is then static -- as a runtime test it was if-converted into
    // selects that doubled the accumulators)
    f64x4 aA[2], aB[2];
    lreg_gemm_for<MB, 0>(wave, Lr, Kl, lane, aA, aB);
    if (saved != nullptr) {
      // training: A (fp32, as the reference casts it) in the adjoint's LDS tile layout, so
      // gpk_var_adjs_l_kernel needs neither the forward GEMM nor the K_ZX Gram again
      float* sb = saved + (size_t)t * LSaved<MB>::blk;
#pragma unroll
      for (int ct = 0; ct < 2; ++ct) {
        *(f32x4*)(sb + ((rA * 2 + ct) * 64 + lane) * 4) =
            f32x4{(float)aA[ct][0], (float)aA[ct][1], (float)aA[ct][2], (float)aA[ct][3]};
        if (rB != rA)
          *(f32x4*)(sb + ((rB * 2 + ct) * 64 + lane) * 4) =
              f32x4{(float)aB[ct][0], (float)aB[ct][1], (float)aB[ct][2], (float)aB[ct][3]};
      }
    }
    // partials over the wave's rows (A cast to fp32 as the reference does)
#pragma unroll
    for (int ct = 0; ct < 2; ++ct) {
      float mp = 0.f, vp = 0.f;
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rowA = 16 * rA + g + 4 * r;
        const float a = (float)aA[ct][r];
        mp = __builtin_fmaf(a, vm[rowA], mp);
        vp = __builtin_fmaf(a * a, sm1[rowA], vp);
      }
      if (rB != rA) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int rowB = 16 * rB + g + 4 * r;
          const float a = (float)aB[ct][r];
          mp = __builtin_fmaf(a, vm[rowB], mp);
          vp = __builtin_fmaf(a * a, sm1[rowB], vp);
        }
      }
      mp += __shfl_xor(mp, 16, 64);
      mp += __shfl_xor(mp, 32, 64);
      vp += __shfl_xor(vp, 16, 64);
      vp += __shfl_xor(vp, 32, 64);
      if (g == 0) {
        red[(wave * 2 + 0) * LTW + 16 * ct + c] = mp;
        red[(wave * 2 + 1) * LTW + 16 * ct + c] = vp;
      }
    }
    lds_barrier();
    if (tid < nvalid) {
      float mm = 0.f, vv = 0.f;
#pragma unroll
      for (int q = 0; q < NWV; ++q) {
        mm += red[(q * 2 + 0) * LTW + tid];
        vv += red[(q * 2 + 1) * LTW + tid];
      }
      const float mean_i = mm + (lin[tid] + b0);
      float var_i = s2 + jit + vv;
      const bool clamp = var_i < 1e-6f;
      if (clamp) { var_i = 1e-6f; clamped = 1; }  // MVN.variance clamp (fp32)
      mean_out[(size_t)b * N + i0 + tid] = mean_i;
      var_out[(size_t)b * N + i0 + tid] = var_i;
      // the clamp passes no gradient: the adjoint masks gvar with this
      if (saved != nullptr) saved[(size_t)t * LSaved<MB>::blk + LSaved<MB>::tiles + tid] = clamp ? 0.f : 1.f;
    } else if (saved != nullptr && tid < LTW) {
      saved[(size_t)t * LSaved<MB>::blk + LSaved<MB>::tiles + tid] = 0.f;
    }
  }
  if (flags != nullptr && clamped)
    (void)__hip_atomic_fetch_or(flags, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

template <int MB, int DQ>
int launch_var_fwd_l(const GpkVarArgs& a, int* flags, hipStream_t stream) {
  using G = LGeo<MB, DQ>;
  const size_t lds = (size_t)G::total * sizeof(float);
  if (lds > 160 * 1024) return -11;
  set_lds_once<gpk_var_fwd_l_kernel<MB, DQ>>();
  const long long nch = (long long)a.B * ((a.N + LTW - 1) / LTW);
  if (nch > 0x7fffffffLL) return -8;
  const int per_cu = G::NWV <= 4 ? 2 : 1;   // <= 2 waves per SIMD (256 VGPRs: L^{-1} resident)
  // the training forward keeps A for the adjoint when the saved-state adjoint serves this shape
  float* saved = (a.saved != nullptr && var_saved_path<MB, DQ>(a.M)) ? a.saved : nullptr;
  hipLaunchKernelGGL((gpk_var_fwd_l_kernel<MB, DQ>), dim3(chunk_grid(nch, per_cu), a.O), dim3(G::NT), lds,
                     stream, a.X, a.Z, a.Linv, a.vmean, a.vstd, a.hyp, a.N, a.M, a.D, (int)nch,
                     a.mean, a.var, flags, saved, fwd_strides(a));
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) return (int)e;
  return a.ell != nullptr ? gpk_launch_var_ell(a, stream) : 0;
}

}  // namespace

int gpk_launch_var_fwd_l(const GpkVarArgs& a, int* flags, hipStream_t stream) {
#define GPK_CALL_FWDL(mb)                                                     \
  if (a.D <= 16) return launch_var_fwd_l<mb, 16>(a, flags, stream);           \
  if (a.D <= 32) return launch_var_fwd_l<mb, 32>(a, flags, stream);           \
  return launch_var_fwd_l<mb, 64>(a, flags, stream);
  const int mb = (a.M + 15) / 16;
  if (mb <= 6) { GPK_CALL_FWDL(6) }
  if (mb <= 8) { GPK_CALL_FWDL(8) }
  if (mb <= 12) { GPK_CALL_FWDL(12) }
  if (mb <= 16) { GPK_CALL_FWDL(16) }
#undef GPK_CALL_FWDL
  return -10;
}
