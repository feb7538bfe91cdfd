// Host arithmetic of the GEMM launchers (gemm.hip): which kernel, how many K slices, which grid.  Plain C++17 -- no HIP, no common.hpp -- so that the same
// code that steers every dense launch also builds with the host compiler: tests/gemm_plan_main.cpp runs it under AddressSanitizer + UBSan.  The launchers
// AND the plan queries (alm_gemm_nt_plan, alm_gemm_tn_batched_plan, ...) call these functions: one source of truth per decision.
#pragma once
#include <cmath>
#include <cstdint>
#include <cstdlib>

#include "../../include/audiolm_hip.h"

#ifdef __HIPCC__
#define ALM_PLAN_HD __host__ __device__ __forceinline__
#else
#define ALM_PLAN_HD inline
#endif

namespace gemm_plan {

constexpr int BK = 64;

// Every A/B environment hook of gemm.hip, read ONCE (gemm_env()).  Name: default -- meaning:
//   ALM_GEMM_BIG_TILE: 0 -- 2 / 11 / 13 / 14: that tile for every big launch (11 never where the caller's panel arithmetic is in 256 x 256 tiles)
//   ALM_GEMM_NT_STORE: 0 -- non-temporal C stores: 1 = always, 2 = bf16 outputs only
//   ALM_GEMM_W4_MINK: 0 (off) -- routes the automatic 256 x 256 choices with at least that many K elements per slice to the 4-wave tile (gemm_w4_kernel, id
//     14).  OPT-IN: stand-alone its main loop is 4-9 % faster per K-step than the staggered tile on long contractions (K = 1024 -1 %, 2736 +-0, 5472 +4 %,
//     8192 +6-9 %), but INSIDE the training step it measured slower on alternating runs (4096: NT big-tile time 3.94 -> 4.05 ms / step; 2048: 4.13 ms; TN
//     unchanged) -- one wave per SIMD has nothing to cover a late operand fetch with when the inputs come from HBM instead of a warm L2
//   ALM_GEMM_W4_TN_MINK: 8192 (0: off) -- ... except the full-K weight-gradient launches of the hybrid plan (TN, K = all tokens of the batch, no slices): there
//     the 4-wave tile is ON -- its longer uninterrupted main loop is what it was built for: -0.05 ms / step on three interleaved runs
//   ALM_GEMM_MID_TILE: 0 -- 1 routes the automatic small-tile choices with N >= 512 and >= 192 such tiles to tile 15 (round 5 experiment, NT only): 256 x 128,
//     8 waves as 4 x 2 (wave tile 64 x 64), one workgroup per CU -- for the N = 512 projections (Wq forward, dAO): 64 x 4 = 256 tiles = ONE round of the chip
//     where the 128 x 128 tile runs 512 workgroups at twice the L2 -> LDS bytes per flop
//   ALM_GEMM_RING: 1 (0: off) -- tile 16 (round 5): the 128 x 128 tile with a 4-stage DMA ring, for NT launches of so few tiles that every CU holds at most one
//     workgroup anyway (to_kv: 128) -- there the two-stage loop waits for one memory round trip per K-step
//   ALM_GEMM_GROUP_M: 0 (= 8) -- rasterisation group of a raster-0 launch (GemmParams::group_m); negative = groups of tile columns
//   ALM_GEMM_T320_COST: 122 (x 100; 0 = never) -- relative cost of the 320 x 256 tile in pick_tile's round model
//   ALM_GEMM_NT_INL: 1 -- in-launch split-K of under-filled NT launches (nt_plan): 0 = off, 1 = cost model, >= 2 = that many slices wherever they fit
//   ALM_GEMM_HYBRID: 1 (0: the uniform split-K plan) / ALM_GEMM_HYBRID_RASTER: 2 (1 = round-robin) -- the hybrid full-K + tail plan of the batched weight
//     gradients / the XCD placement of its panels (2 = a contiguous block per XCD)
//   ALM_GEMM_GROUP2: 1 (0: two launches) -- alm_gemm_bf16_nt_group2 as ONE launch.  ALM_GEMM_GROUP2_BIG: 0 -- round 6, measured and NOT adopted: two problems
//     that are each too small for the big tile (< 192 tiles of 256 x 256) but TOGETHER fill the chip in one round on the staggered tile (dXN_q || dX_kv at
//     M = 8192: 128 + 128 tiles) -- 23.1 us against 22.3 us on the 128 x 128 tile (profiles/r6b_group2.log): K = 512 / 128 is 8 / 2 K-steps, fill + drain dominate
//   ALM_PACK_WIDE: 1 -- alm_pack_weights_multi on the 16-byte-both-ways kernel (0 = the round-2 kernels)
struct GemmEnv {
    int big_tile = 0, nt_store = 0, w4_mink = 0, w4_tn_mink = 8192, mid_tile = 0, ring = 1, group_m = 0, nt_inl = 1, hybrid = 1, hybrid_raster = 2, group2 = 1,
        group2_big = 0, pack_wide = 1;
    double t320_cost = 1.22;
};
inline const GemmEnv& gemm_env() {
    static const GemmEnv env = [] {
        GemmEnv e;
        const auto get = [](const char* name, int* v) { if (const char* s = std::getenv(name)) *v = std::atoi(s); };
        get("ALM_GEMM_BIG_TILE", &e.big_tile); get("ALM_GEMM_NT_STORE", &e.nt_store); get("ALM_GEMM_W4_MINK", &e.w4_mink); get("ALM_GEMM_W4_TN_MINK", &e.w4_tn_mink);
        get("ALM_GEMM_MID_TILE", &e.mid_tile); get("ALM_GEMM_RING", &e.ring); get("ALM_GEMM_GROUP_M", &e.group_m); get("ALM_GEMM_NT_INL", &e.nt_inl);
        get("ALM_GEMM_HYBRID", &e.hybrid); get("ALM_GEMM_HYBRID_RASTER", &e.hybrid_raster); get("ALM_GEMM_GROUP2", &e.group2); get("ALM_GEMM_GROUP2_BIG", &e.group2_big);
        get("ALM_PACK_WIDE", &e.pack_wide);
        if (const char* s = std::getenv("ALM_GEMM_T320_COST")) e.t320_cost = std::atoi(s) / 100.0;
        return e;
    }();
    return env;
}

// Tile ids (alm_gemm_bf16_nt_tile): 1 = 128 x 128 (4 waves, two workgroups per CU), 2 = 256 x 256 lock-step (8 waves), 13 = 256 x 256 with
// staggered wave rows (the production big tile), 11 = 384 x 256 (8 waves, wave tile 192 x 64: 17 % fewer L2 -> LDS bytes per flop), 17 = 320 x 256 (round 6).
// Automatic choice (tile 0): small problems -> 1; otherwise 13, except that an NT problem takes 11 when the coarser tiling needs so many
// fewer rounds of 256 resident workgroups that it wins despite its 1.5x longer tile (measured per-tile cost ratio 1.41: W1 forward
// 16384 x 5472: 6 rounds -> 4, +6 %; with N = 1024 it is 172 tiles on 256 CUs, -15 %).
inline int pick_tile(int M, int N, int ny, int tile, bool tn, const GemmEnv& e = gemm_env()) {
    if (tile == 1 || tile == 2 || tile == 11 || tile == 13 || tile == 14 || tile == 15 || tile == 16 || tile == 17) return tile;
    if (tile != 0) return -1;
    if (M < 256 || N < 256) return 1;
    const long long t256 = (long long)((M + 255) / 256) * ((N + 255) / 256) * ny;
    if (t256 < 192) return 1;               // not enough 256^2 tiles to occupy most of the 256 CUs
    if (!tn) {
        // round model over the three big tiles: rounds of 256 resident workgroups x measured cost of one tile relative to 256 x 256 (384 x 256: 1.41).  Round 6:
        // 320 x 256 (tile 17, the generic 8-wave kernel with a 160 x 64 wave tile) for RAGGED token counts -- FineTransformer N = 2049, B = 8: M = 16 392 is 65 tile
        // rows of 256, so an N = 1024 output is 260 tiles = TWO rounds; 384 x 256 makes it 172 tiles (one round at 67 % of the CUs), 320 x 256 makes it 208
        // (one round at 81 %, shorter tiles).  GemmEnv::t320_cost is its relative cost in the model.
        const double c320 = e.t320_cost;
        const long long t384 = (long long)((M + 383) / 384) * ((N + 255) / 256) * ny;
        const long long t320 = (long long)((M + 319) / 320) * ((N + 255) / 256) * ny;
        const double c13 = (double)((t256 + 255) / 256), c11 = (double)((t384 + 255) / 256) * 1.41;
        const double c17 = c320 > 0. ? (double)((t320 + 255) / 256) * c320 : 1e30;
        if (c17 < c13 && c17 < c11) return 17;
        if (c11 < c13) return 11;
    }
    return 13;
}

// The FINAL tile id of one launch (launch_gemm switches on it; alm_gemm_nt_plan asks it with the arguments alm_gemm_bf16_nt passes), < 0: unsupported.
// tile: the requested id (0 = automatic); kslice: K elements per slice (K when the launch is not split); hook: the A/B hooks apply; only256: the caller's
// panel arithmetic (GemmParams.plimit and the tail offset of the hybrid weight-gradient plan) is in units of 256 x 256 tiles -- the hook may swap the
// 256 x 256 kernels for one another there, never re-tile the launch (a 384 x 256 grid would cover the wrong set of C tiles).
inline int final_tile(bool tn, int M, int N, int kslice, int ny, int nz, int tile, bool hook, bool only256, bool split, int raster, const GemmEnv& e = gemm_env()) {
    int tl = pick_tile(M, N, ny * nz, tile, tn, e);
    if (tl < 0) return -1;
    if (hook && tl != 1 && (e.big_tile == 2 || e.big_tile == 13 || e.big_tile == 14 || (e.big_tile == 11 && !only256))) tl = e.big_tile;
    if (hook && e.w4_mink > 0 && tl == 13 && tile == 0 && kslice >= e.w4_mink) tl = 14;
    if (tn && hook && e.w4_tn_mink > 0 && tl == 13 && kslice >= e.w4_tn_mink) tl = 14;
    if (!tn && hook && e.mid_tile && tl == 1 && tile == 0 && !split && M >= 256 && N >= 512 && (long long)((M + 255) / 256) * ((N + 127) / 128) * ny >= 192) tl = 15;
    const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128) * ny * nz;
    if (!tn && hook && e.ring && tl == 1 && tile == 0 && !split && raster == 0 && kslice >= 256 && t128 <= 256) tl = 16;
    if ((tl == 16 && (tn || raster != 0)) || (tl == 17 && tn)) return -1;
    return tl;
}

inline bool view_too_big(long long rows, long long ld) { return rows * ld * 2 >= 0x7fffffffLL; }

// Operand checks of the entry points.  strides: the OR of the entry point's batch strides (0: none); rows_a / rows_b: rows of the largest A / B view one
// workgroup addresses (384 / 256 for the tile forms, 256 / 256 for NT split-K; TN: the whole contraction)
inline int nt_operands_ok(const void* A, const void* B, int K, long long lda, long long ldb, long long strides, long long rows_a, long long rows_b) {
    if (K <= 0 || (K & 7) || (lda & 7) || (ldb & 7) || (strides & 7) || ((uintptr_t)A & 15) || ((uintptr_t)B & 15)) return ALM_ERR_BAD_ARG;
    return view_too_big(rows_a, lda) || view_too_big(rows_b, ldb) ? ALM_ERR_UNSUPPORTED : 0;
}
inline int tn_operands_ok(const void* At, const void* Bt, int K, long long lda, long long ldb, long long strides) {
    if (K <= 0 || (lda & 7) || (ldb & 7) || (strides & 7) || ((uintptr_t)At & 15) || ((uintptr_t)Bt & 15)) return ALM_ERR_BAD_ARG;
    return view_too_big(K, lda) || view_too_big(K, ldb) ? ALM_ERR_UNSUPPORTED : 0;
}

// K cut into `slices` slices of whole K-steps: kc elements each, nsl of them non-empty; and the grid of the reduce over mn output elements
struct SplitGeometry { int kc, nsl; };
inline SplitGeometry split_geometry(int K, int slices) {
    const int kc = ((K + slices - 1) / slices + BK - 1) / BK * BK;
    return SplitGeometry{kc, (K + kc - 1) / kc};
}
inline int reduce_grid(long long mn) { return (int)((mn + 255) / 256 < 2048 ? (mn + 255) / 256 : 2048); }

// ---- NT launches that cannot fill the chip with 256 x 256 tiles (round 6): in-launch split-K on the staggered tile ----------------------------------------
// pick_tile() sends every NT launch with < 192 tiles of 256 x 256 to the 128 x 128 tile (twice the L2 -> LDS bytes per flop).  With a caller-owned workspace
// the alternative is the staggered 256 x 256 tile with each tile's K range cut over S workgroups (gemm_stag_inl_kernel): tiles x S <= 256 workgroups = ONE
// resident round of the chip.  MEASURED on MI355X (scripts/ab_nt_inl.py, every launch on a fresh operand set; profiles/r6a_nt_inl_cost.log, r6b_*):
//   * a half-empty chip is NOT half as fast: one K-step of a 256 x 256 workgroup takes 1.2 us with 32 workgroups in flight, 1.6 us with 128, 2.0 us with 256
//     (L2 / fabric contention), so cutting K in two over twice the workgroups saves ~35 %, not 50 %, of the main loop;
//   * the publish + reduce is a BURST: every workgroup ends at the same time and writes its 256-KiB slab through to memory -- 16 us with 128 workgroups (32 MB),
//     24 us with 256 (64 MB) -- and the 128 x 128 tile it competes with runs at 0.25-0.31 of the MFMA peak on these shapes (2 workgroups per CU, all CUs busy).
//   Net: the split wins only on LONG contractions -- M = 8192, N = 1024, K = 5472 (dXN = dU W1): 116 -> 107 us; K = 2736: 66 vs 68 us (tie); K <= 1024: the
//   128 x 128 tile wins by 1.5-2x (to_q at M = 16384: 24.5 vs 45.6 us).  A 256 x 128 tile (one round of 256 workgroups for N = 1024) measured 0-14 % SLOWER than
//   the 128 x 128 tile on every shape.  The model below reproduces those decisions; its constants are the fitted ones:
//     t(256^2, S >= 2) = ceil(ksteps / S) * (1.15 + 0.0033 W) + 7 + (8 + 0.04 W) + 2.6 * slabs read        [us; W = tiles x S workgroups]
//     t(128^2)         = rounds of 512 resident workgroups * (ksteps * 1.31 + 4.5)   |   <= 256 tiles (4-stage ring form): ksteps * 0.72 + 4.5
// Workspace: [1024 ticket counters, zero when handed over -- the kernel leaves them zero][tiles x S slabs of 256 KiB].
constexpr long long INL_CNT_BYTES = 4096, INL_SLAB_BYTES = 256 * 256 * 4;
struct NtPlan { int tile, slices; };
inline NtPlan nt_plan(int M, int N, int K, int nb, const GemmEnv& e = gemm_env()) {
    const int mode = e.nt_inl;
    const int base = pick_tile(M, N, nb, 0, false, e);
    if (mode == 0 || base != 1 || M < 256 || N < 256) return NtPlan{base, 1};
    const long long t256 = (long long)((M + 255) / 256) * ((N + 255) / 256) * nb;
    const long long t128 = (long long)((M + 127) / 128) * ((N + 127) / 128) * nb;
    if (t256 > 128) return NtPlan{base, 1};                                     // (two slices must fit one resident round)
    const int ksteps = (K + BK - 1) / BK;
    double best_t = t128 <= 256 ? ksteps * 0.72 + 4.5 : (double)((t128 + 511) / 512) * (ksteps * 1.31 + 4.5);
    NtPlan best{base, 1};
    for (int S = 2; S <= 8; ++S) {
        const long long W = t256 * S;
        if (W > 256) break;
        const int kc = (ksteps + S - 1) / S;
        if (kc < 4) break;
        if ((ksteps + kc - 1) / kc != S) continue;                              // (no empty slices)
        const double t = kc * (1.15 + 0.0033 * W) + 7.0 + (8.0 + 0.04 * W) + 2.6 * (S == 2 ? 1 : S);
        if (mode >= 2 ? (S == mode || best.slices == 1) : t < best_t) { best_t = t; best = NtPlan{13, S}; }
    }
    return best;
}

// What alm_gemm_bf16_nt_ws (with_ws) / alm_gemm_bf16_nt launches for nb problems (alm_gemm_nt_plan).  Without an in-launch split the launch is
// launch_gemm<false>(p, nb, 1, out_f32, 0, st): final_tile with exactly those arguments, on the SHIPPED choice -- the BIG_TILE / W4_MINK / MID_TILE hooks are
// not applied, RING and NT_INL are
struct NtQuery { int tile, slices; long long ws_bytes, wgs; };
inline NtQuery nt_query(int M, int N, int K, int nb, bool with_ws, const GemmEnv& e = gemm_env()) {
    const NtPlan pl = with_ws ? nt_plan(M, N, K, nb, e) : NtPlan{0, 1};
    GemmEnv shipped = e;
    shipped.big_tile = shipped.w4_mink = shipped.mid_tile = 0;
    const int tile = pl.slices > 1 ? pl.tile : final_tile(false, M, N, K, nb, 1, 0, true, false, false, 0, shipped);
    const long long bm = tile == 11 ? 384 : (tile == 17 ? 320 : (tile == 13 ? 256 : 128)), bn = tile == 1 || tile == 16 ? 128 : 256;
    const long long wgs = ((M + bm - 1) / bm) * ((N + bn - 1) / bn) * nb * pl.slices;
    return NtQuery{tile, pl.slices, pl.slices > 1 ? INL_CNT_BYTES + wgs * INL_SLAB_BYTES : 0, wgs};
}

// Split-K plan for `nb` same-shape problems: choose (tile, slices) minimising a simple time model --
//   block waves over the chip x K-steps per block x measured time per K-step  +  workspace round trip through HBM.
// (A balanced "stream-K"-like split -- one equally long K-step range per CU -- measured SLOWER: the workgroups of an XCD then walk different
// K ranges and no longer share operand panels through the L2; it lives in csrc/lab/gemm_lab.hip)
struct SplitPlan { int tile, slices; };

// XCD-panel rasterisation pays only when the panels spread evenly over the 8 XCDs (measured: 22 panels +3 %, 11 panels -40 %)
inline int pick_raster(int M, int N, int nb, int tile) {
    const int bm = tile >= 2 ? 256 : 128;
    const int tmm = (M + bm - 1) / bm, tnn = (N + bm - 1) / bm;
    const int P = (tmm >= tnn ? tmm : tnn) * nb;
    return (P % 8 == 0 || P >= 20) ? 1 : 0;
}
inline SplitPlan splitk_plan(int M, int N, int K, int nb) {
    SplitPlan best{1, 1};
    double best_t = 1e30;
    for (int tile = 1; tile <= 2; ++tile) {
        if (tile == 2 && (M < 256 || N < 256)) continue;
        const int bm = tile == 2 ? 256 : 128;
        const double tiles = (double)((M + bm - 1) / bm) * ((N + bm - 1) / bm) * nb;
        const double slots = tile == 2 ? 256.0 : 512.0;               // resident blocks on the chip
        const double us_per_kstep = tile == 2 ? 2.0 : 1.25;          // one 64-deep K-step of one block (measured, whole chip busy)
        for (int s = 1; s <= 64; ++s) {
            if (s > 1 && (K + s - 1) / s < 256) break;
            const SplitGeometry g = split_geometry(K, s);
            if (g.nsl != s) continue;
            const double waves = std::ceil(tiles * s / slots);
            double t = waves * ((g.kc / BK) * us_per_kstep + 3.0);
            if (s > 1) t += (double)s * M * N * nb * 8.0 / 4.0e6 + 3.0;   // fp32 partials: written + read back at ~4 TB/s, + the reduce launch
            if (t < best_t) { best_t = t; best = SplitPlan{tile == 2 ? 13 : 1, s}; }
        }
    }
    return best;
}

// Hybrid plan of the layer-batched weight gradients (alm_gemm_bf16_tn_batched): when the 256 x 256 tiles of all problems fill the chip's 256 CUs a
// whole number of times plus a SMALL remainder (dW1 of 3 layers: 264 tiles), the uniform split-K plan pays for the remainder with partials of
// EVERYTHING (4 slices: 5 waves of K/4 + 270 MB of fp32 partials).  Instead: the first panels_a panels (whole waves) run at full K straight into C,
// and the remaining row (column) blocks -- they all lie in the LAST problem -- are one ordinary split-K launch, sliced deep enough to occupy the chip
// once.  panels_a == 0: not applicable (use the uniform plan).
struct HybridPlan { int panels_a, m_major, off, slices_b; };
inline HybridPlan hybrid_plan(int M, int N, int K, int nb, const GemmEnv& e = gemm_env()) {
    HybridPlan none{0, 0, 0, 0};
    if (!e.hybrid || M < 256 || N < 256 || K < 4096) return none;
    const int tm = (M + 255) / 256, tn = (N + 255) / 256;
    const int m_major = tm >= tn, tmaj = m_major ? tm : tn, Q = m_major ? tn : tm;
    const int P = tmaj * nb, total = P * Q;
    if (total <= 256) return none;
    const int panels_a = (total / 256) * 256 / Q;                 // whole waves of 256 tiles (Q tiles per panel)
    const int rem = P - panels_a;
    if (panels_a * Q % 256 != 0 || rem <= 0 || rem >= tmaj || rem * Q > 64) return none;    // the tail must be small and inside the last problem
    const int off = (tmaj - rem) * 256;
    int s = 256 / (rem * Q);                                      // tail tiles x slices ~ one wave of the chip
    const int ksteps = (K + BK - 1) / BK;
    while (s > 1 && ksteps / s < 8) --s;                          // at least 8 K-steps per slice
    if (s < 2) return none;
    return HybridPlan{panels_a, m_major, off, s};
}

// fp32 workspace floats of alm_gemm_bf16_{nt,tn}_splitk and alm_gemm_bf16_tn_batched (the hybrid tail's partials: the larger of the two covers both callers)
inline long long splitk_ws_floats(int M, int N, int K, int nb, const GemmEnv& e = gemm_env()) {
    const SplitPlan pl = splitk_plan(M, N, K, nb);
    long long fl = pl.slices > 1 ? (long long)pl.slices * nb * M * N : 0;
    const HybridPlan hy = hybrid_plan(M, N, K, nb, e);
    if (hy.panels_a > 0) {
        const long long m2 = hy.m_major ? M - hy.off : M, n2 = hy.m_major ? N : N - hy.off;
        const long long f2 = (long long)hy.slices_b * m2 * n2;
        if (f2 > fl) fl = f2;
    }
    return fl;
}

// ---- plan of the grouped leftover launch (gemm_tn_grouped_kernel) ------------------------------------------------------------------------------------
// ONE slice count S for all jobs, from a time model in the form of the measured NT one (docs/LABBOOK.md round 6, item 2: us = 9.0 + 1.52 ksteps + 18.1 (S > 1) + 2.6 S per
// launch of one resident round), re-fitted to this launch at the headline's leftovers (144 tiles, K = 16384, S = 1 .. 10; docs/LABBOOK.md round 7):
//   t(S) = full rounds x (TNG_ROUND_US + TNG_KSTEP_US x kps)  +  last, partial round: TNG_ROUND_US + kps x (TNG_KSTEP_LO_US + (TNG_KSTEP_US - TNG_KSTEP_LO_US) x f)
//          +  [S > 1]  (TNG_PUBLISH_US + (S + 1) x leftover bytes / TNG_REDUCE_BPUS)
// kps = K-steps per slice; rounds = the busiest XCD's workgroups / its 32 CUs, f = the filled fraction of the last one (a K-step of a 256 x 256 workgroup takes
// 1.2 us on a nearly empty chip and 1.9 us on a full one: a part-filled last round is cheaper than a whole one).  Reproduces the ten measured totals to 7 %
// and their order (S = 5 at the headline shape).  Slices are whole K-steps, none empty, at least 4 K-steps each.
constexpr double TNG_ROUND_US = 9.0, TNG_KSTEP_US = 1.92, TNG_KSTEP_LO_US = 1.2, TNG_PUBLISH_US = 18.1, TNG_REDUCE_BPUS = 5.8e6;
constexpr int TN_GROUP_MAX = 8;
struct TnGroupPlan { int tiles, S, kps, pieces, blocks, rounds; long long ws_floats; int longest; };
// where every live job's units sit: the placement arrays of the kernel's table (TnGroupTable in gemm.hip, which explains them; the launcher copies them)
struct TnGroupPlacement { int tiles[TN_GROUP_MAX], tiles_n[TN_GROUP_MAX], nunits[TN_GROUP_MAX], base[TN_GROUP_MAX], njobs, S; };

// workgroups of XCD x's list that belong to a job whose units are [base, base + n): those numbered == x (mod 8); `first` = the lowest of them
ALM_PLAN_HD int tn_group_units_on(int base, int n, int x, int* first) {
    const int f = base + ((x - base) & 7);
    *first = f;
    return f < base + n ? (base + n - 1 - f) / 8 + 1 : 0;
}

inline bool tn_job_live(const AlmTnJob& j) { return j.M > 0 && j.N > 0 && j.nb1 > 0 && j.nb2 > 0; }
inline int tn_jobs_check(const AlmTnJob* jobs, int njobs) {
    if (njobs < 0 || njobs > TN_GROUP_MAX || (njobs > 0 && !jobs)) return ALM_ERR_BAD_ARG;
    int K = 0;
    for (int i = 0; i < njobs; ++i) {
        const AlmTnJob& j = jobs[i];
        if (!tn_job_live(j)) continue;
        if (j.K <= 0 || (K && j.K != K)) return ALM_ERR_BAD_ARG;            // one contraction length per call
        K = j.K;
        if (const int rc = tn_operands_ok(j.At, j.Bt, j.K, j.lda, j.ldb, j.sA1 | j.sA2 | j.sB1 | j.sB2)) return rc;
        if ((long long)j.nb1 * j.nb2 > 4096 || j.M > (1 << 23) || j.N > (1 << 23)) return ALM_ERR_UNSUPPORTED;
    }
    return 0;
}

// geometry of the launch for a GIVEN S: fills tiles / pieces / blocks / rounds / ws_floats (and the placement when pc != nullptr)
inline void tn_group_geometry(const AlmTnJob* jobs, int njobs, int S, TnGroupPlan* pl, TnGroupPlacement* pc) {
    TnGroupPlacement g;
    int base = 0, nj = 0, tiles = 0;
    long long wsf = 0;
    for (int i = 0; i < njobs; ++i) {
        const AlmTnJob& j = jobs[i];
        if (!tn_job_live(j)) continue;
        const int tm = (j.M + 255) / 256, tn = (j.N + 255) / 256, nbt = j.nb1 * j.nb2;
        g.tiles[nj] = tm * tn; g.tiles_n[nj] = tn; g.nunits[nj] = nbt * S; g.base[nj] = base;
        base += nbt * S;
        tiles += tm * tn * nbt;
        if (S > 1) wsf += ((long long)S * nbt * j.M * j.N + 3) & ~3LL;      // (every job's partials start 16-byte aligned)
        ++nj;
    }
    g.njobs = nj; g.S = S;
    int longest = 0;
    for (int x = 0; x < 8; ++x) {
        int len = 0, first;
        for (int k = 0; k < nj; ++k) len += tn_group_units_on(g.base[k], g.nunits[k], x, &first) * g.tiles[k];
        longest = len > longest ? len : longest;
    }
    pl->tiles = tiles; pl->S = S; pl->pieces = tiles * S; pl->blocks = 8 * longest; pl->rounds = (longest + 31) / 32; pl->ws_floats = wsf; pl->longest = longest;
    if (pc) *pc = g;
}

// K-steps per slice when K is cut into S slices of whole K-steps, or 0 when that leaves a slice empty
inline int tn_group_kps(int K, int S) {
    const int ksteps = (K + BK - 1) / BK, kps = (ksteps + S - 1) / S;
    return (ksteps + kps - 1) / kps == S ? kps : 0;
}

inline TnGroupPlan tn_group_plan(const AlmTnJob* jobs, int njobs, int slices) {
    TnGroupPlan best{0, 1, 0, 0, 0, 0, 0, 0};
    int K = 0;
    double elems = 0.;
    for (int i = 0; i < njobs; ++i)
        if (tn_job_live(jobs[i])) { K = jobs[i].K; elems += (double)jobs[i].nb1 * jobs[i].nb2 * jobs[i].M * jobs[i].N; }
    if (K == 0) return best;
    if (slices > 0) {                                                       // forced: the nearest count at or below it that leaves no slice empty
        int S = slices;
        while (S > 1 && tn_group_kps(K, S) == 0) --S;
        tn_group_geometry(jobs, njobs, S, &best, nullptr);
        best.kps = tn_group_kps(K, S);
        return best;
    }
    double best_t = 1e30;
    for (int S = 1; S <= 32; ++S) {
        const int kps = tn_group_kps(K, S);
        if (kps == 0 || (S > 1 && kps < 4)) continue;
        TnGroupPlan pl;
        tn_group_geometry(jobs, njobs, S, &pl, nullptr);
        pl.kps = kps;
        if (pl.ws_floats > 0x7fffffffLL) break;
        const int full = pl.longest / 32;
        const double f = (pl.longest % 32) / 32.0;
        double t = full * (TNG_ROUND_US + TNG_KSTEP_US * kps);
        if (f > 0.) t += TNG_ROUND_US + kps * (TNG_KSTEP_LO_US + (TNG_KSTEP_US - TNG_KSTEP_LO_US) * f);
        if (S > 1) t += TNG_PUBLISH_US + (S + 1) * elems * 4.0 / TNG_REDUCE_BPUS;
        if (t < best_t) { best_t = t; best = pl; }
    }
    return best;
}

}  // namespace gemm_plan
