// Stand-alone check of csrc/gemm_plan.hpp, the host arithmetic that decides which kernel every dense launch runs: built by tests/test_gemm_plan_host.py with
// the host compiler and -fsanitize=address,undefined (no HIP), run as a child process.  Exit code 0 and "ok" = every check held.
#include <cstdio>
#include <vector>

#include "gemm_plan.hpp"

using namespace gemm_plan;

#define CHECK(cond)                                                                                        \
    do {                                                                                                   \
        if (!(cond)) {                                                                                     \
            std::printf("FAILED line %d: %s   [M %d N %d K %d nb %d S %d]\n", __LINE__, #cond, cM, cN, cK, cnb, cS); \
            return 1;                                                                                      \
        }                                                                                                  \
    } while (0)

static int cM, cN, cK, cnb, cS;              // the case at hand, printed by a failing CHECK
static const int MN[] = {1, 64, 127, 128, 129, 255, 256, 257, 300, 512, 1024, 1025, 2730, 2736, 5472, 8192, 16384, 16392, 16448};
static const int KS[] = {8, 64, 200, 256, 1024, 2736, 4096, 16384, 131072};
static const int NB[] = {1, 2, 3, 6, 12, 24};

static long long cdiv(long long a, long long b) { return (a + b - 1) / b; }

static AlmTnJob job(int M, int N, int K, int nb1, int nb2) {
    AlmTnJob j{};
    j.M = M; j.N = N; j.K = K; j.nb1 = nb1; j.nb2 = nb2; j.alpha = 1.f;
    j.lda = (M + 7) / 8 * 8; j.ldb = (N + 7) / 8 * 8; j.ldc = N;
    return j;
}

// (1) the decisions tests/test_plan_queries.py pins at the headline shapes: D 1024, heads 8 x 64, FFN inner 2730 (padded 2736), 6 layers, M = K = 16384
static int pins() {
    const GemmEnv e{};
    const int D = 1024, HD = 512, DH2 = 128, I = 2730, IP = 2736, L = 6, M = 8 * 2048, K = 8 * 2048;
    CHECK(pick_tile(M, HD, 1, 0, false, e) == 1 && pick_tile(M, DH2, 1, 0, false, e) == 1);
    CHECK(pick_tile(M, D, 1, 0, false, e) == 13);
    CHECK(pick_tile(M, 2 * IP, 1, 0, false, e) == 11 && pick_tile(M, IP, 1, 0, false, e) == 11);
    CHECK(pick_tile(8 * 512, 1025, 3, 0, false, e) == 13 && pick_tile(8 * 509, 501, 1, 0, false, e) == 1);
    for (int N : {HD, DH2, D, 2 * IP, IP}) CHECK(pick_tile(2048, N, 1, 0, false, e) == 1);
    HybridPlan h = hybrid_plan(I, D, K, 2 * L, e);               // dW1: 12 problems, 528 tiles: 512 at full K, tail = the last 4 row blocks
    CHECK(h.panels_a == 128 && h.m_major == 1 && h.off == (11 - 4) * 256 && h.slices_b >= 8);
    h = hybrid_plan(D, I, K, L, e);                              // dW2: 6 problems, 264 tiles: 256 at full K, tail = the last 2 column blocks
    CHECK(h.panels_a == 64 && h.m_major == 0 && h.off == (11 - 2) * 256 && h.slices_b >= 8);
    const int small[3][2] = {{D, HD}, {HD, D}, {DH2, D}};        // dWo / dWq / dWkv: uniform split-K
    for (auto& s : small) CHECK(hybrid_plan(s[0], s[1], K, L, e).panels_a == 0 && splitk_plan(s[0], s[1], K, L).slices > 1);
    CHECK(hybrid_plan(I, D, 2048, 2 * L, e).panels_a == 0);      // B = 1: below the hybrid plan's 4096 floor
    return 0;
}

// (2) invariants of the NT / split-K / hybrid plans over the sweep, and (4) launch and query agree on the ring tile
static int sweep(const GemmEnv& e) {
    for (int M : MN) for (int N : MN) for (int K : KS) for (int nb : NB) {
        cM = M; cN = N; cK = K; cnb = nb;
        const long long t256 = cdiv(M, 256) * cdiv(N, 256) * nb, ksteps = cdiv(K, BK);
        // in-launch split-K of an NT launch
        const NtPlan np = nt_plan(M, N, K, nb, e);
        const NtQuery q1 = nt_query(M, N, K, nb, true, e), q0 = nt_query(M, N, K, nb, false, e);
        cS = np.slices;
        CHECK(np.slices >= 1 && np.slices <= 8 && q1.slices == np.slices && q0.slices == 1 && q0.ws_bytes == 0);
        if (np.slices > 1) {
            const long long kc = cdiv(ksteps, np.slices);        // K-steps per slice, as nt_launch_ws cuts them
            CHECK(np.tile == 13 && q1.tile == 13 && M >= 256 && N >= 256);
            CHECK(kc >= 4 && cdiv(K, kc * BK) == np.slices);     // whole K-steps, none empty: inl_slices == S
            CHECK(t256 * np.slices <= 256 && q1.wgs == t256 * np.slices);
            CHECK(q1.ws_bytes == INL_CNT_BYTES + t256 * np.slices * INL_SLAB_BYTES && q1.ws_bytes <= INL_CNT_BYTES + 256 * INL_SLAB_BYTES);
        } else {
            CHECK(q1.ws_bytes == 0 && q1.tile == q0.tile);
        }
        // the final tile of the automatic launch = the tile the query names (the hooks the query leaves out never touch tile 1 / 16)
        const int ft = final_tile(false, M, N, K, nb, 1, 0, true, false, false, 0, e);
        GemmEnv shipped = e;
        shipped.big_tile = shipped.w4_mink = shipped.mid_tile = 0;
        CHECK((ft == 16) == (q0.tile == 16) && q0.tile == final_tile(false, M, N, K, nb, 1, 0, true, false, false, 0, shipped));
        CHECK(q0.tile != 16 || (e.ring && K >= 256 && cdiv(M, 128) * cdiv(N, 128) * nb <= 256));
        if (np.slices == 1) CHECK((ft == 16) == (q1.tile == 16));
        // uniform split-K
        const SplitPlan sp = splitk_plan(M, N, K, nb);
        const SplitGeometry g = split_geometry(K, sp.slices);
        cS = sp.slices;
        CHECK(sp.slices >= 1 && sp.slices <= 64 && (sp.tile == 1 || sp.tile == 13));
        CHECK(g.nsl == sp.slices && g.kc % BK == 0 && (long long)(g.nsl - 1) * g.kc < K && (long long)g.nsl * g.kc >= K);
        const long long wsf = splitk_ws_floats(M, N, K, nb, e);
        CHECK(wsf >= (sp.slices > 1 ? (long long)g.nsl * nb * M * N : 0));
        // hybrid full-K + tail
        const HybridPlan h = hybrid_plan(M, N, K, nb, e);
        if (h.panels_a > 0) {
            const int tm = (int)cdiv(M, 256), tn = (int)cdiv(N, 256), tmaj = h.m_major ? tm : tn, Q = h.m_major ? tn : tm, rem = tmaj * nb - h.panels_a;
            cS = h.slices_b;
            CHECK(e.hybrid && h.m_major == (tm >= tn) && h.panels_a * Q % 256 == 0);
            CHECK(rem > 0 && rem < tmaj && h.off == (tmaj - rem) * 256 && h.off > 0 && h.off < (h.m_major ? M : N));      // the tail lies inside the last problem
            const SplitGeometry gt = split_geometry(K, h.slices_b);                  // what splitk_fixed launches
            CHECK(h.slices_b >= 2 && gt.nsl >= 1 && gt.nsl <= h.slices_b && gt.kc % BK == 0 && (long long)(gt.nsl - 1) * gt.kc < K && (long long)gt.nsl * gt.kc >= K);
            const long long m2 = h.m_major ? M - h.off : M, n2 = h.m_major ? N : N - h.off;
            CHECK(wsf >= gt.nsl * m2 * n2);
        }
    }
    return 0;
}

// (3) the grouped plan: every (job, problem, slice, tile) on exactly one (XCD list, slot), found the way gemm_tn_grouped_kernel finds it from blockIdx.x
static int grouped_case(const std::vector<AlmTnJob>& jobs) {
    const int n = (int)jobs.size();
    for (int S = 1; S <= 32; ++S) {
        cS = S; cnb = n;
        TnGroupPlan pl;
        TnGroupPlacement g;
        tn_group_geometry(jobs.data(), n, S, &pl, &g);
        long long pieces = 0, wsf = 0;
        int live = 0;
        std::vector<std::vector<char>> seen;
        for (const AlmTnJob& j : jobs) {
            if (!tn_job_live(j)) continue;
            const int tiles = (int)(cdiv(j.M, 256) * cdiv(j.N, 256)), units = j.nb1 * j.nb2 * S;
            CHECK(g.tiles[live] == tiles && g.tiles_n[live] == cdiv(j.N, 256) && g.nunits[live] == units);
            seen.emplace_back((size_t)tiles * units, 0);
            pieces += (long long)tiles * units;
            if (S > 1) wsf += ((long long)units * j.M * j.N + 3) & ~3LL;
            ++live;
        }
        CHECK(g.njobs == live && g.S == S && pl.pieces == pieces && pl.tiles * S == pieces && pl.ws_floats == wsf);
        CHECK(pl.blocks == 8 * pl.longest && pl.rounds == (pl.longest + 31) / 32);
        long long placed = 0, longest = 0;
        for (int b = 0; b < pl.blocks; ++b) {                    // the kernel's walk
            const int x = b & 7;
            int slot = b >> 3, j = 0, first = 0;
            for (; j < g.njobs; ++j) {
                const int p = tn_group_units_on(g.base[j], g.nunits[j], x, &first) * g.tiles[j];
                if (slot < p) break;
                slot -= p;
            }
            if (j >= g.njobs) continue;                          // (the shorter XCD lists)
            const int v = first + 8 * (slot / g.tiles[j]) - g.base[j], t = slot % g.tiles[j];
            CHECK(v >= 0 && v < g.nunits[j] && t >= 0 && t < g.tiles[j] && (g.base[j] + v) % 8 == x);
            char& c = seen[j][(size_t)v * g.tiles[j] + t];
            CHECK(c == 0);
            c = 1;
            ++placed;
            longest = (b >> 3) + 1 > longest ? (b >> 3) + 1 : longest;
        }
        CHECK(placed == pieces && longest == pl.longest);
    }
    // the chosen / forced slice counts: whole K-steps, none empty, at least 4 K-steps each when chosen
    if (tn_jobs_check(jobs.data(), n) == 0) {
        int K = 0;
        for (const AlmTnJob& j : jobs) if (tn_job_live(j)) K = j.K;
        for (int slices = 0; slices <= 33; ++slices) {
            const TnGroupPlan pl = tn_group_plan(jobs.data(), n, slices);
            cS = slices;
            if (K == 0) { CHECK(pl.tiles == 0 && pl.S == 1); continue; }
            CHECK(pl.S >= 1 && (slices == 0 ? pl.S <= 32 : pl.S <= slices) && pl.kps == tn_group_kps(K, pl.S) && pl.kps > 0);
            CHECK((long long)pl.S * pl.kps * BK >= K && (long long)(pl.S - 1) * pl.kps * BK < K && (slices > 0 || pl.S == 1 || pl.kps >= 4));
        }
    }
    return 0;
}

static int grouped() {
    const int K = 16384;
    if (grouped_case({})) return 1;
    if (grouped_case({job(0, 512, K, 1, 1), job(512, 512, K, 0, 3)})) return 1;                      // only empty jobs
    if (grouped_case({job(938, 1024, K, 1, 1)})) return 1;                                          // one job (the dW1 tail)
    if (grouped_case({job(300, 257, 200, 2, 3)})) return 1;
    if (grouped_case({job(938, 1024, K, 1, 1), job(0, 8, K, 1, 1), job(1024, 426, K, 1, 1), job(1024, 512, K, 1, 6), job(512, 1024, K, 6, 1),
                      job(128, 1024, K, 2, 3)})) return 1;                                          // the headline's leftovers + an empty job
    if (grouped_case({job(256, 256, 4096, 1, 1), job(257, 256, 4096, 1, 2), job(1, 1, 4096, 3, 1), job(1300, 700, 4096, 1, 1), job(512, 2730, 4096, 2, 2),
                      job(127, 129, 4096, 1, 5), job(2730, 1024, 4096, 1, 1), job(300, 300, 4096, 7, 1)})) return 1;      // eight jobs of unequal tile counts
    std::vector<AlmTnJob> bad(9, job(256, 256, K, 1, 1));
    CHECK(tn_jobs_check(bad.data(), 9) == ALM_ERR_BAD_ARG && tn_jobs_check(bad.data(), 8) == 0 && tn_jobs_check(nullptr, 1) == ALM_ERR_BAD_ARG);
    bad[1].K = 4096;
    CHECK(tn_jobs_check(bad.data(), 2) == ALM_ERR_BAD_ARG);
    bad[1].K = K; bad[1].lda = 257;
    CHECK(tn_jobs_check(bad.data(), 2) == ALM_ERR_BAD_ARG);
    bad[1].lda = 1LL << 30;
    CHECK(tn_jobs_check(bad.data(), 2) == ALM_ERR_UNSUPPORTED);
    return 0;
}

// the reroutes of final_tile, the operand checks, the slice geometry
static int rules() {
    GemmEnv e{};
    CHECK(final_tile(false, 256, 256, 256, 1, 1, 0, true, false, false, 0, e) == 16 && final_tile(false, 256, 256, 128, 1, 1, 0, true, false, false, 0, e) == 1);
    CHECK(final_tile(false, 256, 256, 256, 1, 1, 0, false, false, false, 0, e) == 1 && final_tile(false, 256, 256, 256, 1, 1, 1, true, false, false, 0, e) == 1);
    CHECK(final_tile(false, 2176, 2048, 128, 1, 1, 0, true, false, false, 0, e) == 1 && final_tile(false, 256, 256, 256, 1, 2, 0, true, false, true, 0, e) == 1);
    CHECK(final_tile(true, 256, 256, 256, 1, 1, 16, true, false, false, 0, e) < 0 && final_tile(true, 256, 256, 256, 1, 1, 17, true, false, false, 0, e) < 0);
    CHECK(final_tile(false, 256, 256, 256, 1, 1, 16, true, false, false, 1, e) < 0 && final_tile(false, 256, 256, 256, 1, 1, 5, true, false, false, 0, e) < 0);
    CHECK(final_tile(true, 2730, 1024, 16384, 12, 1, 13, true, true, false, 2, e) == 14 && final_tile(true, 2730, 1024, 4096, 12, 4, 13, true, false, true, 1, e) == 13);
    CHECK(final_tile(false, 16384, 1024, 16384, 1, 1, 0, true, false, false, 0, e) == 13);              // (W4_TN_MINK is for TN launches only)
    e.w4_mink = 4096;
    CHECK(final_tile(false, 16384, 1024, 4096, 1, 1, 0, true, false, false, 0, e) == 14 && final_tile(false, 16384, 1024, 4096, 1, 1, 13, true, false, false, 0, e) == 13);
    CHECK(final_tile(false, 16384, 1024, 4096, 1, 1, 0, false, false, false, 0, e) == 13 && nt_query(16384, 1024, 4096, 1, true, e).tile == 13);
    e = GemmEnv{}; e.big_tile = 11;
    CHECK(final_tile(true, 2730, 1024, 1024, 12, 1, 13, true, true, false, 2, e) == 13 && final_tile(true, 2730, 1024, 1024, 12, 1, 13, true, false, false, 1, e) == 11);
    CHECK(final_tile(false, 256, 256, 256, 1, 1, 0, true, false, false, 0, e) == 16 && nt_query(16384, 1024, 512, 1, false, e).tile == 13);
    e = GemmEnv{}; e.mid_tile = 1;
    CHECK(final_tile(false, 16384, 512, 1024, 1, 1, 0, true, false, false, 0, e) == 15 && nt_query(16384, 512, 1024, 1, false, e).tile == 1);
    e = GemmEnv{}; e.t320_cost = 0.;
    CHECK(pick_tile(16392, 1024, 1, 0, false, GemmEnv{}) == 17 && pick_tile(16392, 1024, 1, 0, false, e) != 17);
    alignas(16) static char buf[32];
    CHECK(nt_operands_ok(buf, buf + 16, 64, 64, 64, 0, 384, 256) == 0 && nt_operands_ok(buf, buf, 12, 64, 64, 0, 384, 256) == ALM_ERR_BAD_ARG);
    CHECK(nt_operands_ok(buf, buf + 8, 64, 64, 64, 0, 384, 256) == ALM_ERR_BAD_ARG && nt_operands_ok(buf, buf, 64, 64, 64, 4, 384, 256) == ALM_ERR_BAD_ARG);
    CHECK(nt_operands_ok(buf, buf, 64, 3LL << 20, 64, 0, 384, 256) == ALM_ERR_UNSUPPORTED && nt_operands_ok(buf, buf, 64, 3LL << 20, 64, 0, 256, 256) == 0);
    CHECK(tn_operands_ok(buf, buf, 12, 64, 64, 0) == 0 && tn_operands_ok(buf, buf, 0, 64, 64, 0) == ALM_ERR_BAD_ARG && tn_operands_ok(buf, buf, 12, 60, 64, 0) == ALM_ERR_BAD_ARG);
    CHECK(tn_operands_ok(buf, buf, 1 << 20, 1024, 64, 0) == ALM_ERR_UNSUPPORTED);
    CHECK(reduce_grid(1) == 1 && reduce_grid(256 * 2048LL) == 2048 && reduce_grid(1LL << 40) == 2048 && reduce_grid(257) == 2);
    CHECK(split_geometry(16384, 5).kc == 3328 && split_geometry(16384, 5).nsl == 5 && split_geometry(100, 1).kc == 128);
    return 0;
}

int main() {
    if (pins() || rules() || grouped()) return 1;
    GemmEnv envs[8];                                             // the defaults and the A/B settings the decisions depend on
    envs[1].ring = 0; envs[2].nt_inl = 0; envs[3].nt_inl = 2; envs[4].hybrid = 0; envs[5].t320_cost = 0.; envs[6].big_tile = 13; envs[7].w4_mink = 4096;
    for (const GemmEnv& e : envs)
        if (sweep(e)) return 1;
    std::printf("ok\n");
    return 0;
}
