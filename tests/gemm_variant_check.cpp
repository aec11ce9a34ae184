// The k_gemm launch variants (sacx_internal.h: GemmRows, gemm_variant_ok, gemm_workgroups) against
// tables written out by hand from the launcher they replaced; built and run by
// tests/test_abi.py::test_gemm_variant_table
#include "sacx_internal.h"
#include <cstdio>
#include <random>
using namespace sacx;

// The branches the hand-written ladders of launch_gemm_t / launch_gemm had: the value each tested for
// in each mode, and whether that branch existed on 32x32 tiles and for packed seeds
struct Row { int mode, rows; bool t32, packed; };
static const Row kTable[] = {
    {GM_FWD, 0, true, true},      // k_gemm<GM_FWD, V, 0, 4, BF, PK, T32>
    {GM_FWD, 3, false, true},     // k_gemm_head<V, Q, BF, PK> (launch_gemm: 16x16 tiles only)
    {GM_FWD, 5, true, true},
    {GM_FWD, 6, false, false},    // <.., false, false> alone
    {GM_FWD, 8, true, true},
    {GM_DX, 0, true, true},
    {GM_DX, 1, true, true},
    {GM_DX, 2, true, true},
    {GM_DX, 4, false, true},      // <.., PK, false>
    {GM_DX, 7, false, false},     // <.., false, false> alone
    {GM_DW, 0, true, true},
    {GM_DW, 3, true, true},
    {GM_FWD2, 0, false, false},   // k_fwd2: one seed, 16x16 MFMA tiles
    {GM_FWD2, 3, false, false},
    {GM_FWD2, 5, false, false},
    {GM_FWD2, 6, false, false},
    {GM_FWD2, 9, false, false},
};
static bool expect_ok(int mode, int rows, bool t32, bool packed, int dwl) {
    // k_dwl<BF, PK, NH>: plain dW + Adam problems on its own 32-row tiles, one seed or packed
    if (dwl) return mode == GM_DW && rows == 0 && !t32;
    for (const Row& r : kTable)
        if (r.mode == mode && r.rows == rows) return (!t32 || r.t32) && (!packed || r.packed);
    return false;
}

int main() {
    int bad = 0;
    // 1. the values are part of the kernel names
    static_assert(GR_NONE == 0 && GR_QHEAD == 1 && GR_PIQHEAD == 2 && GR_ACTOR_HEAD == 3 && GR_POLICY_HEAD == 3 &&
                      GR_PAIR_HEAD == 3 && GR_HEAD_BWD == 4 && GR_HEAD_PART == 5 && GR_GATHER == 6 && GR_GEN_BWD2 == 7 &&
                      GR_MSE_HEAD == 8 && GR_PREGATHERED == 9 && GR_COUNT == 10,
                  "GemmRows values");
    static_assert(GM_FWD == 0 && GM_DX == 1 && GM_DW == 2 && GM_FWD2 == 3, "GemmMode values");
    static_assert(sizeof(GemmRows) == sizeof(int32_t), "GemmRows is an int32_t");
    // 2. the whole product mode x value x tiles x packing x k_dwl form
    int cases = 0, accepted = 0;
    for (int mode = 0; mode < 4; ++mode)
        for (int rows = 0; rows < 10; ++rows)
            for (int t32 = 0; t32 < 2; ++t32)
                for (int pk = 0; pk < 2; ++pk)
                    for (int dwl = 0; dwl < 3; ++dwl) {
                        const bool got = gemm_variant_ok(mode, rows, t32 != 0, pk != 0, dwl);
                        const bool want = expect_ok(mode, rows, t32 != 0, pk != 0, dwl);
                        ++cases;
                        accepted += got;
                        if (got != want) {
                            ++bad;
                            printf("variant_ok(mode %d, rows %d, t32 %d, packed %d, dwl %d) = %d, expected %d\n", mode, rows, t32,
                                   pk, dwl, (int)got, (int)want);
                        }
                    }
    // (the accepted count, by hand: FWD 4 + 2 + 4 + 1 + 4, DX 4 + 4 + 4 + 2 + 1, DW 4 + 4, FWD2 5, k_dwl 2 x 2)
    if (accepted != 15 + 15 + 8 + 5 + 4) { ++bad; printf("accepted %d of %d\n", accepted, cases); }
    bad += gemm_variant_ok(4, 0, false, false, 0) || gemm_variant_ok(-1, 0, false, false, 0) ||
           gemm_variant_ok(GM_FWD, 10, false, false, 0) || gemm_variant_ok(GM_DW, 0, false, false, 3);
    // 3. the launcher's four grid formulas, as they stood
    std::mt19937 r(2);
    int draws = 0;
    for (const Row& row : kTable) {
        if (row.mode == GM_FWD2) continue;      // (k_fwd2's grid is 2-D: launch_gemm's own)
        for (int it = 0; it < 3000; ++it, ++draws) {
            GemmArgs a{};
            a.mode = row.mode; a.rowk = row.rows;
            a.total_tiles = r() % 5000; a.row_blocks = r() % 600; a.has_final = r() % 3; a.has_mfinal = r() % 3;
            const int grid = a.total_tiles + (a.has_final ? 1 : 0) + (a.has_mfinal ? 1 : 0);
            int want;
            if (a.mode == GM_FWD) {
                const int gh = a.total_tiles + (a.has_final ? 1 : 0) + a.row_blocks;
                want = a.rowk == 3 ? gh : grid;
            } else if (a.mode == GM_DX) {
                const int gx = a.total_tiles + (a.rowk && a.rowk < 3 ? a.row_blocks : 0) + (a.has_mfinal ? 1 : 0);
                want = gx;
            } else {
                const int gh = a.total_tiles + a.row_blocks;
                want = a.rowk == 3 ? gh : grid;
            }
            if (gemm_workgroups(a) != want) {
                if (bad < 20) printf("workgroups(mode %d rows %d tiles %d rb %d fin %d mfin %d) = %d, expected %d\n", a.mode,
                                     a.rowk, a.total_tiles, a.row_blocks, a.has_final, a.has_mfinal, gemm_workgroups(a), want);
                ++bad;
            }
        }
    }
    printf("gemm variants: %d combinations, %d grid draws, %d mismatches\n", cases, draws, bad);
    return bad != 0;
}
