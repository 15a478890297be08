// tools/exp/exp_hooks.inc -- the experiment side of emdr2_amd/csrc/exp_hooks.h: compiled only by `make exp` (-DEMDR2_EXPERIMENTS) into
// lib/libemdr2_hip_exp.so, which tools/ load for ablations and knob sweeps; never part of libemdr2_hip.so.  Every switch is read from the
// environment; the product build has none of this (its hooks are empty macros).
#include <stdlib.h>
// ---- gemm.hip: EMDR2_GEMM_ABLATE 1 = no epilogue, 2 = no k-loop, 3 = epilogue without global stores; EMDR2_GEMM_ORDER / _L2_KB tile order;
//      EMDR2_GEMM8=0 keeps the persistent kernel out; EMDR2_GEMM_TILE 22 / 21 / 44 alternative tilings --------------------------------------
#define EXP_GEMM_KLOOP_LEN(p, nch) ((p).ablate == 2 ? 0 : (nch))
#define EXP_GEMM_AFTER_KLOOP(p, acc) if ((p).ablate == 1) { if (acc[0][0][0] == 123.456f) ((float *)(p).C)[0] = acc[1][3][5]; return; }
#define EXP_GEMM_STORE_IF(p, w) if ((p).ablate != 3 || (w)[0] == 0x12345678u)
#define EXP_GEMM_TILE_ORDER(order_env, ablate_env, l2_env) \
    static const int order_env = getenv("EMDR2_GEMM_ORDER") ? atoi(getenv("EMDR2_GEMM_ORDER")) : 1; \
    static const int ablate_env = getenv("EMDR2_GEMM_ABLATE") ? atoi(getenv("EMDR2_GEMM_ABLATE")) : 0; \
    static const int l2_env = getenv("EMDR2_GEMM_L2_KB") ? atoi(getenv("EMDR2_GEMM_L2_KB")) : 2560;
static inline bool exp_gemm_use_gemm8() { static const int v = getenv("EMDR2_GEMM8") ? atoi(getenv("EMDR2_GEMM8")) : 1; return v != 0; }
#define EXP_GEMM_USE_GEMM8() exp_gemm_use_gemm8()
// EMDR2_GEMM_TILE=22: 128 x 256 tiles on 4 waves, two workgroups per CU (one's epilogue overlaps the other's MFMA loop).  Measured 5-8 %
// SLOWER than 256 x 256 on the step's linears (1.5x the L2->LDS operand traffic per flop).  =44: 256 x 256 tile on FOUR waves of 128 x 128
// (256 accumulator registers per lane, one wave per SIMD): 8 fragment reads per 16 MFMAs instead of 6 per 8 -> a third less LDS read traffic
#define EXP_GEMM_TILE_VARIANTS(p, batch, split_k, stream) { \
    static const int tile_env = getenv("EMDR2_GEMM_TILE") ? atoi(getenv("EMDR2_GEMM_TILE")) : 42; \
    if (tile_env == 22 && split_k == 1) return launch_gemm<2, 2>(p, batch, (hipStream_t)stream); \
    if (tile_env == 21 && split_k == 1) return launch_gemm<2, 1>(p, batch, (hipStream_t)stream); \
    if (tile_env == 44 && split_k == 1) return launch_gemm<2, 2, 4>(p, batch, (hipStream_t)stream); }
// ---- gemm8.hip: EMDR2_G8_ABLATE 1 = no epilogue, 2 = epilogue without global stores; _SINGLE_KB / _NGROUP / _NT / _STAGGER ---------------
#define EXP_G8_AFTER_KLOOP(p, acc, wr) if ((p).ablate == 1) { \
    _Pragma("unroll") for (int mi = 0; mi < 8; ++mi) _Pragma("unroll") for (int ni = 0; ni < 4; ++ni) asm volatile("" ::"v"(acc[mi][ni])); \
    if (wr == 1) { PIPE_BARRIER(); } continue; }
#define EXP_G8_STORE_IF(p, w) if ((p).ablate != 2 || (w)[0] == 0x12345678u)
#define EXP_G8_HOST_L2(single_kb) { static const int single_env = getenv("EMDR2_G8_SINGLE_KB") ? atoi(getenv("EMDR2_G8_SINGLE_KB")) : 0; if (single_env > 0) single_kb = single_env; }
#define EXP_G8_HOST_GROUPS(p, ng) { static const int ng_env = getenv("EMDR2_G8_NGROUP") ? atoi(getenv("EMDR2_G8_NGROUP")) : 0; \
    if (ng_env > 0) ng = ng_env; \
    static const int nt_env = getenv("EMDR2_G8_NT") ? atoi(getenv("EMDR2_G8_NT")) : 0; (p).nt_a = nt_env; }
#define EXP_G8_HOST_LAUNCH(p) { static const int ablate_env = getenv("EMDR2_G8_ABLATE") ? atoi(getenv("EMDR2_G8_ABLATE")) : 0; \
    static const int stagger_env = getenv("EMDR2_G8_STAGGER") ? atoi(getenv("EMDR2_G8_STAGGER")) : -1; \
    (p).ablate = ablate_env; if (stagger_env >= 0) (p).stagger = stagger_env; }
// ---- gemm8t.hip: EMDR2_T8_ABLATE 1 = the DMA stream re-reads its first K-tile (always L2-hot), 2 = no DMA at all, 3 = every slice streams
//      slice 0's rows; gemm_tn.hip: EMDR2_TN_OLD=1 keeps the persistent weight-gradient kernel out -----------------------------------------------
#define EXP_T8_STREAM(p, zs, KT, zs_addr, KT_STREAM, T8_DMA_ON) \
    const int zs_addr = (p).ablate == 3 ? 0 : zs; const int KT_STREAM = (p).ablate == 1 ? 1 : KT; const bool T8_DMA_ON = (p).ablate != 2;
#define EXP_T8_HOST(p) { static const int ablate_env = getenv("EMDR2_T8_ABLATE") ? atoi(getenv("EMDR2_T8_ABLATE")) : 0; (p).ablate = ablate_env; }
#define EXP_TN_GENERAL_ONLY(general_only) { static const bool tn_old = getenv("EMDR2_TN_OLD") && atoi(getenv("EMDR2_TN_OLD")); general_only = tn_old; }
// ---- MIPS: EMDR2_MIPS_SEG0 / _GROWTH / _VARIANT / _GRID / _KERNEL / _ABLATE / _TUNE / _COUPLE (mips_api.hip), schedule variants
//      (tools/exp/mips_scan_variants*.inc), the filter-never-fires and late-start timing switches of the persistent scan (EXP_SCAN8_*: they
//      sit in the kernel template of csrc/mips_scan8.h and so act on its fp16 AND its int8 instance) --------------------------------------------
static inline int exp_env_int(const char *name, int dflt) { const char *v = getenv(name); return (v && *v) ? atoi(v) : dflt; }
#define EXP_ENV_INT(name, dflt) exp_env_int(name, dflt)
#define EXP_MIPS_PACK_QUERIES_FRAG(variant, scan_kernel, qp, nqp, dim, w, stream, rc) \
    if (variant == 0 && scan_kernel == 5 && (rc = mips_launch_pack_queries_frag(qp, nqp, dim, (w).q_frag, stream))) return rc;
#define EXP_MIPS_COUPLE() (exp_env_int("EMDR2_MIPS_COUPLE", 1) != 0)
// (in front of the launch of a LOCKSTEP segment of the plan: with any of these switches set, mips_plan.h gives every segment behind the dense one that engine)
#define EXP_MIPS_SCAN_VARIANT(variant, ablate, scan_kernel, sp, w, grid, seg_end, n_rows, done, stream, rc) \
    if (variant == 0 && ablate > 0) rc = mips_launch_scan_ablate(ablate, sp, grid, stream); \
    else if (variant == 0 && scan_kernel == 5) { ScanParams sq = sp; sq.q_tiled = (w).q_frag; rc = mips_launch_scan_q8(ablate == 53 ? 3 : 0, sq, grid, stream); } \
    else if (scan_kernel == 2) rc = mips_launch_scan_pp(variant, 3, sp, grid, stream); \
    else if (scan_kernel == 4) rc = mips_launch_scan_pp(variant, seg_end == n_rows && done >= n_rows / 16 ? 4 : 3, sp, grid, stream); \
    else
#define EXP_SCAN8_TAU(p, tauv, qt) if ((p).tune & 128) tauv[qt] = __builtin_inff();        /* timing experiment: the filter never fires */
#define EXP_SCAN8_LATE_START(P, hq) if (hq == 1) for (int i = 0; i < (P).s.tune >> 8; ++i) __builtin_amdgcn_s_sleep(32);   /* EMDR2_MIPS_TUNE bits 8..: late start of the second half */
