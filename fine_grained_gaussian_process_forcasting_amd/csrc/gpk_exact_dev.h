// Build switches and development-only instrumentation of the exact kernel (gpk_exact_kernel.h,
// compiled by the gpk_exact_nb*.hip units).
//
// Product builds (build_native.py) define none of these macros: the switch below defaults
// to the shipped, measured setting; the knockouts compile to `false`; the stamp macros only
// expand inside kernels instantiated with STAMPS = true (the gpk_debug_exact_stamps entry,
// scripts/stamps_exact.py). A/B builds: scripts/ab_build_one.sh <name> 'gpk_exact_nb*.hip' -DNAME=v
// (every unit that includes this header; build_native.build_variant does the same).
#pragma once

// ---- the one design switch left: both sides ship (build_native.VARIANTS["f32update"]) ----
#ifndef GPK_SPLIT_UPDATE
#define GPK_SPLIT_UPDATE 1   // 1: split-f16 trailing update; 0: pure fp32 MFMA (bench.py's fp32_update note)
#endif
constexpr int kWorkerPrio = 1;   // workers raise their issue priority to this from the right-hand side through
                                 // the TRSM and for the hand-over (2.5 % + ~2 % per launch, profiles/r03_exact_prio_ab.txt)
constexpr int kLStoreAux = 17;   // cache policy of the L buffer stores (sc0 sc1: write-through, the lines leave L2)

// Retired switches: one line each, what was tried; the losing sides are gone from the source and
// the measured verdicts stay in DESIGN.md §4.1 and the named record under profiles/.
//   GPK_EXACT_WBIG=16        16 waves at two windows per CU for NB >= 12 (8 kept)
//   GPK_EXACT_SMALLB=0       no one-window-per-CU, 16-wave layout for B <= CUs (r04_exact_ab.jsonl)
//   GPK_EXACT_DIAG_ALONE=0   15 workers at NB <= 8 instead of the diagonal wave alone on its SIMD
//                            (r06_exact_alone_ab.txt, r06_exact_alone13_ab.txt)
//   GPK_EXACT_PRIO=0         no raised worker priority; GPK_EXACT_PRIO_RHS=0: raised only at the TRSM
//                            (r03_exact_prio_ab.txt)
//   GPK_DIAG_DPP=0           diagonal sweep as readlane broadcasts into pinned SGPRs (r03_mb_diag.txt)
//   GPK_DIAG_PERMLANE=1      sweep operand by permlane swaps from the look-ahead's registers: slower
//                            than through the LDS tile; GPK_DIAG_FINISH_LATE=1: step k's L block and
//                            log|T| behind the look-ahead MFMAs: slower (r06_exact_ab.txt)
//   GPK_EXACT_COL=0          split-barrier plan at N = 256 with 8 waves
//   GPK_LST_AUX=-1           plain global L stores, 64.5 vs 59.2 us per B = 512 launch

// ---- development only ----
#ifndef GPK_EXACT_DEV
#define GPK_EXACT_DEV 0   // 1: only the N = 128 / 256 instantiations (fast A/B compiles): units without
                          // NB = 8 or 16 compile to a launcher that returns -6 (launch_exact_case)
#endif
#ifndef GPK_TMO_DEBUG
#define GPK_TMO_DEBUG 0   // 1 (debug builds): a timed-out window's info = flag index | target << 8
#endif
#ifndef GPK_EPOCH_CHECK
#define GPK_EPOCH_CHECK 0   // 1 (check builds): every consumed panel / hand-over / R_kk^{-T} tile is checked
                            // against the epoch its consumer expects (epoch shadows in LDS, written by the
                            // producer before its flag release); a mismatch ends the window with
                            // info = 1<<20 and the site in flag word kFlagEpochBad. 2: the same plus a
                            // deliberate wrong mark (the check's own negative control).
#endif
constexpr bool kEpochCheck = GPK_EPOCH_CHECK != 0;
#if GPK_EPOCH_CHECK
#define GPK_EP(...) __VA_ARGS__
#else
#define GPK_EP(...)
#endif
constexpr bool kEpochSabotage = GPK_EPOCH_CHECK == 2;
#ifndef GPK_KO
#define GPK_KO 0   // knockout bits (timing only, results WRONG): see the constants below
#endif
constexpr bool kKoTrsmMfma = (GPK_KO & 1) != 0;       // TRSM MFMAs
constexpr bool kKoRhs = (GPK_KO & 2) != 0;            // right-hand side
constexpr bool kKoZeroL = (GPK_KO & 4) != 0;          // upper-L zeroing
constexpr bool kKoDeferredRbf = (GPK_KO & 8) != 0;    // deferred RBF of block row k + 2
constexpr bool kKoBulkUpdate = (GPK_KO & 16) != 0;    // bulk trailing update
constexpr bool kKoTrsmLStores = (GPK_KO & 32) != 0;   // TRSM L stores
constexpr bool kKoDiagSweep = (GPK_KO & 64) != 0;     // diagonal sweep
constexpr bool kKoOneOperand = (GPK_KO & 128) != 0;   // one LDS operand per tile update
constexpr bool kKoAny = GPK_KO != 0;                  // (disables the failure checks too)

// ---- stamp builds (STAMPS = true instantiations only) ----
constexpr int kStampStride = 32 + 16 * 8 * 8;  // phase clocks + per-step timeline

// Diagnostic phase clock inside the worker steps (STAMPS builds only).
#define GPK_WSTAMP(slot, ev)                                      \
  if constexpr (ST) {                                             \
    __builtin_amdgcn_sched_barrier(0);                            \
    const unsigned long long _n = __builtin_amdgcn_s_memtime();   \
    x.st[slot] += _n - x.st[8];                                   \
    x.st[8] = _n;                                                 \
    if (x.lane == 0) x.tl[(K * 8 + x.wv) * 8 + (ev)] = _n;        \
    __builtin_amdgcn_sched_barrier(0);                            \
  }

// Phase clock of the kernel body (wave 0 lane 0 of each workgroup).
#define GPK_STAMP(slot)                                           \
  if constexpr (STAMPS) {                                         \
    __builtin_amdgcn_sched_barrier(0);                            \
    const unsigned long long _n = __builtin_amdgcn_s_memtime();   \
    st_acc[slot] += _n - st_last;                                 \
    st_last = _n;                                                 \
    __builtin_amdgcn_sched_barrier(0);                            \
  }
