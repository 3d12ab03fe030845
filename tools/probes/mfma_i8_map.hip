// operand and accumulator lane maps of v_mfma_i32_16x16x64_i8 on gfx950, recovered from one-hot operands (used by ww_q8.hip)
//   1. A one-hot at (lane, byte), B all ones  -> the cells of D that light up are one ROW of D: which, and is it whole?
//   2. B one-hot at (lane, byte), A all ones  -> one COLUMN of D
//   3. A one-hot in row 0 and B one-hot in column 0 -> D[0][0] lights up exactly when the two bytes carry the same k
// The absolute k of a byte cannot be observed (a product sums over k); what a kernel needs is 3: which A byte meets which B byte.
// Rows and columns of D are named by the C/D map every 16x16 MFMA has: cell (row, col) is register row & 3 of lane
// 16 (row >> 2) + col.  Prints a markdown block (tools/probes/mfma_i8_map.py puts it into DESIGN.md).
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <string.h>
#include <vector>
typedef int v4i __attribute__((ext_vector_type(4)));

__device__ v4i one_hot(int lane, int byte, int hot_lane, int hot_byte, bool all_ones) {
    v4i v = {0, 0, 0, 0};
    if (all_ones) { v[0] = v[1] = v[2] = v[3] = 0x01010101; return v; }
    if (lane == hot_lane) {
#pragma unroll
        for (int d = 0; d < 4; ++d)
            if ((hot_byte >> 2) == d) v[d] = 1 << (8 * (hot_byte & 3));
    }
    return v;
}

// mode 0: A one-hot at slot e = lane * 16 + byte, B ones; mode 1: the reverse.  out[e][lane][reg]
__global__ void k_rows_cols(int mode, int *out) {
    const int lane = threadIdx.x;
    for (int e = 0; e < 1024; ++e) {
        const v4i hot = one_hot(lane, 0, e >> 4, e & 15, false), ones = one_hot(lane, 0, 0, 0, true), zero = {0, 0, 0, 0};
        const v4i d = mode == 0 ? __builtin_amdgcn_mfma_i32_16x16x64_i8(hot, ones, zero, 0, 0, 0)
                                : __builtin_amdgcn_mfma_i32_16x16x64_i8(ones, hot, zero, 0, 0, 0);
        for (int r = 0; r < 4; ++r) out[(e * 64 + lane) * 4 + r] = d[r];
    }
}

// A one-hot at (lane 16 ga, byte ja), B one-hot at (lane 16 gb, byte jb): out[(ga*16+ja)*64 + gb*16+jb] = D[0][0]
__global__ void k_pairs(int *out) {
    const int lane = threadIdx.x;
    for (int ea = 0; ea < 64; ++ea)
        for (int eb = 0; eb < 64; ++eb) {
            const v4i a = one_hot(lane, 0, 16 * (ea >> 4), ea & 15, false), b = one_hot(lane, 0, 16 * (eb >> 4), eb & 15, false);
            const v4i zero = {0, 0, 0, 0};
            const v4i d = __builtin_amdgcn_mfma_i32_16x16x64_i8(a, b, zero, 0, 0, 0);
            if (lane == 0) out[ea * 64 + eb] = d[0];
        }
}

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 2; } } while (0)

// which row (mode 0) or column (mode 1) of D slot e lights, -1 unless it is exactly one whole row / column of ones
static int line_of(const int *d, int mode) {
    int line = -1, cells = 0;
    for (int lane = 0; lane < 64; ++lane)
        for (int r = 0; r < 4; ++r) {
            const int v = d[lane * 4 + r];
            if (!v) continue;
            if (v != 1) return -1;
            const int row = 4 * (lane >> 4) + r, col = lane & 15, l = mode == 0 ? row : col;
            if (line >= 0 && l != line) return -1;
            line = l;
            ++cells;
        }
    return cells == 16 ? line : -1;
}

int main() {
    int *d1, *d3;
    std::vector<int> h(1024 * 256), p(4096);
    CK(hipMalloc(&d1, h.size() * sizeof(int)));
    CK(hipMalloc(&d3, p.size() * sizeof(int)));
    int line[2][1024];
    bool lane_only[2] = {true, true};
    for (int mode = 0; mode < 2; ++mode) {
        hipLaunchKernelGGL(k_rows_cols, dim3(1), dim3(64), 0, 0, mode, d1);
        CK(hipMemcpy(h.data(), d1, h.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int e = 0; e < 1024; ++e) {
            line[mode][e] = line_of(&h[e * 256], mode);
            if (line[mode][e] < 0) { printf("FAILED: %s slot lane %d byte %d does not light one whole %s\n", mode ? "B" : "A", e >> 4, e & 15, mode ? "column" : "row"); return 1; }
            lane_only[mode] &= line[mode][e] == ((e >> 4) & 15);
        }
    }
    hipLaunchKernelGGL(k_pairs, dim3(1), dim3(64), 0, 0, d3);
    CK(hipMemcpy(p.data(), d3, p.size() * sizeof(int), hipMemcpyDeviceToHost));
    bool identity = true;
    for (int ea = 0; ea < 64; ++ea)
        for (int eb = 0; eb < 64; ++eb) identity &= p[ea * 64 + eb] == (ea == eb ? 1 : 0);
    printf("`v_mfma_i32_16x16x64_i8`, lane `l`, byte `j` (0..15) of the lane's four operand registers, recovered by "
           "`tools/probes/mfma_i8_map.py` from one-hot operands:\n\n");
    printf("| operand | what lane `l` holds | probe |\n|---|---|---|\n");
    printf("| A (16 x 64) | row `l & 15`, the 16 k of group `l >> 4` | %s |\n",
           lane_only[0] ? "every one of the 1024 (lane, byte) slots lights one whole row of D, row `l & 15`" : "**differs: see the table below**");
    printf("| B (64 x 16) | column `l & 15`, the 16 k of group `l >> 4` | %s |\n",
           lane_only[1] ? "every slot lights one whole column of D, column `l & 15`" : "**differs: see the table below**");
    printf("| k | byte `j` of A lane group `g` meets byte `j'` of B lane group `g'` | %s |\n",
           identity ? "exactly when `g == g'` and `j == j'` (4096 pairs tried)" : "**not the identity: see the table below**");
    printf("| C/D (16 x 16) | register `r` of lane `l` is row `4 (l >> 4) + r`, column `l & 15` | the rows and columns above are whole "
           "and distinct under this map |\n");
    if (!lane_only[0] || !lane_only[1] || !identity) {
        printf("\nslot -> line:\n");
        for (int mode = 0; mode < 2; ++mode)
            for (int e = 0; e < 1024; e += 16) printf("%s lane %2d -> %d\n", mode ? "B" : "A", e >> 4, line[mode][e]);
        for (int ea = 0; ea < 64; ++ea)
            for (int eb = 0; eb < 64; ++eb)
                if (p[ea * 64 + eb]) printf("A (g %d, j %2d) meets B (g %d, j %2d)\n", ea >> 4, ea & 15, eb >> 4, eb & 15);
    }
    return 0;
}
