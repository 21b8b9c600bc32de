// dx0_split.h -- d(layer-0 input) of the f32 mode as SIX bf16 MFMA terms per f32 product:
//     dX[M x N] = A[M x K] W[K x N],   A = dG of layer 0 stored [M][lda] (M = steps x rows, the K = 4R gate pre-activations
//                                      contiguous), W = W_i2h[0] given as THREE bf16 images of W^T (p = 0 hi, 1 mid, 2 lo),
//                                      image p at W3 + p N K, each in blocks of 32 k: [K / 32][N][32], so that the 32 k of
//                                      a column are 64 contiguous bytes and one K step of all columns is one contiguous run
//                                      (with plain [N][K] rows a K step would use half of every 128-byte line it fetches,
//                                      and the L2 -> CU path, not the matrix pipe, would set the pace)
// The three-way split of an f32 value and the six terms that matter are kmajor_bf16.h's; they go through
// v_mfma_f32_16x16x32_bf16 into the SAME f32 accumulator.
// DEFINITION (bit-reproducible results): K runs in ascending steps of 32; within a step the terms of an accumulator come in
// the order of WB_TERM_A / WB_TERM_B (piece of A  x  piece of W, smallest first).
// There is no split-K and there are no slabs: every accumulator sees this one fixed sequence whatever the grid is.
//
// Why this product suits the form better than the weight gradients do:
//   * dG is K-CONTIGUOUS.  The A fragment of the MFMA (8 consecutive k of one row) is 32 contiguous bytes of f32 for a lane:
//     two buffer_load_dwordx4 straight into registers, split there.  No LDS image, transposition or barrier for A
//     (lstm_persist_bwd3.h streams dG the same way).  A wave owns 16 rows x ALL columns of its column block (N = 200: 13
//     column tiles, 52 accumulator registers), so with one column block (N <= 256) every dG value is loaded and split exactly
//     once in the launch; with two (N <= 512, arch2's E = 512) each column block loads and splits all of A again: twice.
//   * W does not move during a step: its three images are made once per step (kernels.h: TransposeJob, riding in the
//     embedding launch) and the kernel does no split work for B at all.
// Workgroup = 256 threads = 4 waves = 64 rows (13 312 rows: 208 workgroups, one round on 256 CUs) x one column block of
// NT column tiles (NT = 13: N <= 208; NT = 16: N <= 256, or two column blocks for N <= 512).
// B path: the three images of the step's 32 k x 16 NT columns are staged through LDS: global -> registers (one whole K
//   step ahead) -> LDS buffer (s + 1) & 1 during step s, ONE barrier per K step.  Rows of 64 bytes (32 k), the 16-byte
//   chunk c of column n at 64 n + 16 (c ^ f((n >> 2) & 3)), f = 0, 2, 3, 1: conflict-free for the ds_read_b128
//   fragment read (its lane groups mix lh and lh + 1: MI355X LDS table) and for the contiguous ds_write_b128.
//   Per wave and K step: 6 NT MFMAs (NT = 13: 1248 matrix-pipe cycles), 3 NT ds_read_b128 (4 waves: half the LDS
//   array's cycles), ~60 VALU instructions of split.
//   (A removed variant had every wave read its B fragments from the L2-resident images itself -- no LDS, no barrier, 4 x
//   the L2 reads -- and measured 2-3 x slower: DESIGN.md section 4.1, profiles/dx0_split_ab.json.)
// A fragments travel through a ring of NVQA_DX_PD K steps per lane (2 PD loads in flight).  The buffer descriptor covers
// exactly the workgroup's rows that exist, so rows past M read as zero without a branch; K % 32 == 0 leaves no K tail.
// The K loop runs whole rounds of PD steps: where K / 32 is no multiple of PD, the last round multiplies up to PD - 1 steps
// of zeros at full cost (K = 32 does the work of K = 128).  Nothing at the step's K = 4R = 2048; a cost for small K only.
// Row skipping (ragged batches) as gemm_f32_body's mseg: with seg_rows % 16 == 0, a 16-row tile whose rows all lie at or
// beyond nrows[segment] is neither computed nor written (its outputs are never read); otherwise everything is computed.
// Workgroup ids are dealt round-robin to the 8 XCDs, and each XCD's L2 holds the 2.4 MB of images once.  With row block =
// workgroup id, a segment of S = seg_rows / 64 row blocks would put its row block p on the same XCDs in every segment
// (B = 512: S = 8, XCD = p), and a ragged batch's skipped trailing row blocks would leave the same XCDs idle all launch
// long.  So, where segments are whole numbers of row blocks (seg_rows % 64 == 0, M % seg_rows == 0), workgroup i of
// segment q = i / S takes that segment's row block (i % S + q) % S: a bijection inside each segment, and the active row
// blocks rotate over the XCDs from segment to segment.  Which workgroup computes a row block changes no bit of it.
#pragma once
#include "kmajor_bf16.h"

namespace nvqa {

struct Dx0SplitArgs {
    const float *A;           // [M][lda]
    const unsigned short *W3; // hi, mid, lo images of W^T, each [K / 32][N][32] bf16
    float *out;               // [M][ldo]
    const int *nrows;         // active rows per group of seg_rows rows of A (NULL: all)
    int seg_rows;
    int lda, ldo, M, N, K;
};

#define NVQA_DX_ROWS 64
#define NVQA_DX_THREADS 256
#define NVQA_DX_BK 32
#define NVQA_DX_PD 4 // K steps of A fragments in flight per lane
#define NVQA_DX_OOB 0x40000000u
// one LDS buffer: 3 images x 256 columns x 64 bytes whatever N is (one staging geometry: every chunk's address is the lane's part
// plus a constant); two buffers = 96 KB, so a CU holds ONE workgroup -- 208 workgroups spread over 208 CUs by construction
#define NVQA_DX_PLANE (256 * 64)
constexpr int dx0_split_lds_bytes() { return 2 * 3 * NVQA_DX_PLANE; }
// column tiles per column block and column blocks for N
inline int dx0_split_nt(int N) { return N <= 208 ? 13 : 16; }
inline int dx0_split_col_blocks(int N) { return N <= 256 ? 1 : 2; }

// the shapes the kernel takes (the host keeps the f32 MFMA route otherwise)
inline bool dx0_split_takes(int M, int N, int K, int lda)
{
    if (M <= 0 || N <= 0 || N > 512 || N % 4 || K <= 0 || K % NVQA_DX_BK || lda % 4 || lda < K) return false;
    if ((size_t)3 * N * K * 2 >= NVQA_DX_OOB || (size_t)NVQA_DX_ROWS * lda * 4 >= NVQA_DX_OOB) return false; // 32-bit buffer offsets
    return true;
}

// 8 consecutive k of one row -> the hi, mid and lo fragments
__device__ __forceinline__ void dx_split8(const wb_u32x4 &u0, const wb_u32x4 &u1, wb_bf16x8 (&p)[3])
{
    wb_u32x2 c0[3], c1[3];
    wb_split4(__builtin_bit_cast(wb_f32x4, u0), c0[0], c0[1], c0[2]);
    wb_split4(__builtin_bit_cast(wb_f32x4, u1), c1[0], c1[1], c1[2]);
#pragma unroll
    for (int pl = 0; pl < 3; ++pl) p[pl] = __builtin_bit_cast(wb_bf16x8, wb_u32x4{c0[pl][0], c0[pl][1], c1[pl][0], c1[pl][1]});
}

template <int NT>
__global__ __launch_bounds__(NVQA_DX_THREADS, 1) void k_dx0_split(Dx0SplitArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char dx_smem[];
    constexpr int PD = NVQA_DX_PD, PLANE = NVQA_DX_PLANE, STAGE = 3 * PLANE, NLD = STAGE / 16 / NVQA_DX_THREADS; // 12 chunks per thread
    constexpr int NCH = (NT + 1) / 2; // the column tiles of a K step in NCH groups of 1 or 2 (the MFMA runs at full rate on one accumulator)
    static_assert(NCH >= 3 && NLD >= NCH && NT <= 16, "the A split rides in the first three groups, every group stages a chunk");
    const int tid = threadIdx.x, lane = tid & 63, li = lane & 15, lh = lane >> 4;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    int rb = blockIdx.x; // row block: rotated inside its segment (header), every rb < gridDim.x since M % seg_rows == 0
    if (g.nrows != nullptr && g.seg_rows > 0 && g.seg_rows % NVQA_DX_ROWS == 0 && g.M % g.seg_rows == 0) {
        const int S = g.seg_rows / NVQA_DX_ROWS, q = rb / S;
        rb = q * S + (rb % S + q) % S;
    }
    const int m0 = rb * NVQA_DX_ROWS, n0 = blockIdx.y * (NT * 16);
    const int K = g.K, nk = K / NVQA_DX_BK;

    // which 16-row tiles are computed (block- and wave-uniform, before any barrier)
    const int r0 = m0 + 16 * wave;
    bool active = r0 < g.M; // (a wave whose tile is not computed still stages B and multiplies zeros; it stores nothing)
    if (g.nrows != nullptr && g.seg_rows > 0 && g.seg_rows % 16 == 0) {
        bool any = false;
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int rw = m0 + 16 * w;
            const bool on = rw < g.M && rw % g.seg_rows < g.nrows[rw < g.M ? rw / g.seg_rows : 0];
            any = any || on;
            if (w == wave) active = on;
        }
        if (!any) return;
    }

    // A: the workgroup's rows that exist, through a descriptor of exactly their bytes.  A K step past the end reads zeros (and
    // the last B stage again, in bounds): the loop below runs whole rounds of PD steps without a branch, and a step past the
    // end adds exact zeros to every accumulator.
    const int rows_here = min(NVQA_DX_ROWS, g.M - m0);
    const __amdgpu_buffer_rsrc_t r_a = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<float *>(g.A + (size_t)m0 * g.lda), 0, (int)(((size_t)(rows_here - 1) * g.lda + K) * 4), 0x00020000);
    const __amdgpu_buffer_rsrc_t r_w =
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned short *>(g.W3), 0, (int)((size_t)3 * g.N * K * 2), 0x00020000);
    const unsigned a_off = active ? (unsigned)(((16 * wave + li) * g.lda + 8 * lh) * 4) : NVQA_DX_OOB;
    wb_u32x4 ring[PD][2];
    auto load_a = [&](int slot, int s) { // K step s >= nk: zeros
        const unsigned off = s < nk ? a_off : NVQA_DX_OOB;
        ring[slot][0] = __builtin_amdgcn_raw_buffer_load_b128(r_a, off, s * (NVQA_DX_BK * 4), 0);
        ring[slot][1] = __builtin_amdgcn_raw_buffer_load_b128(r_a, off + 16u, s * (NVQA_DX_BK * 4), 0);
    };

    // B staging.  A stage is [3 images][256 columns][64 bytes]; its 16-byte chunk tid + 256 i is (image i / 4, column
    // tid / 4 + 64 (i % 4), piece tid % 4 of the 32 k): the lane's part of the address is the same for every i, the rest is
    // uniform and goes into the load's scalar offset / the store's immediate offset.  Columns past N (and past 16 NT) load
    // zeros.  Two register sets: the stage of step s + 1 sits in set (s + 1) & 1 from step s - 2 (global -> registers) to
    // step s (registers -> LDS), so a stage has two whole K steps to arrive.
    wb_u32x4 st[2][NLD];
    unsigned st_goff[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        st_goff[q] = n0 + (tid >> 2) + 64 * q < g.N ? (unsigned)(n0 * 64 + 16 * tid) : NVQA_DX_OOB; // 256 threads: 4 KB in a row
    const unsigned st_loff = (unsigned)((tid >> 2) * 64 + 16 * ((tid & 3) ^ ((0x78 >> (2 * ((tid >> 4) & 3))) & 3)));
    const int img_bytes = g.N * K * 2;
    auto load_b = [&](int set, int i, int s) {
        st[set][i] = __builtin_amdgcn_raw_buffer_load_b128(r_w, st_goff[i & 3], (i >> 2) * img_bytes + (i & 3) * 4096 + min(s, nk - 1) * g.N * 64, 0);
    };
    auto store_b = [&](int set, int i, int buf) {
        *reinterpret_cast<wb_u32x4 *>(dx_smem + buf * STAGE + i * 4096 + st_loff) = st[set][i];
    };
    // fragment of column tile j, image pl: lane (li, lh) holds W^T[16 j + li][8 lh .. 8 lh + 7] of the step
    const unsigned f_loff = (unsigned)(li * 64 + 16 * (lh ^ ((0x78 >> (2 * (li >> 2))) & 3)));
    auto frag_b = [&](int buf, int pl, int j) -> wb_bf16x8 {
        return __builtin_bit_cast(wb_bf16x8, *reinterpret_cast<const wb_u32x4 *>(dx_smem + buf * STAGE + pl * PLANE + j * 1024 + f_loff));
    };

    wb_f32x4 acc[NT];
#pragma unroll
    for (int j = 0; j < NT; ++j) acc[j] = wb_f32x4{0.f, 0.f, 0.f, 0.f};

    // Prologue, in the loop's own load order -- oldest first the ring, then the stages of steps 0 (straight on into LDS), 1
    // and 2 -- and fenced so that it stays in that order: the waits inside the loop are static, and the compiler sets each
    // to the FEWER of the younger loads on the two ways into the loop.  A prologue that left fewer loads behind a register
    // than a round of the loop does would make that wait drain the ring in every round.
#pragma unroll
    for (int p = 0; p < PD; ++p) load_a(p, p);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NLD; ++i) load_b(0, i, 0);
#pragma unroll
    for (int i = 0; i < NLD; ++i) store_b(0, i, 0);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NLD; ++i) load_b(1, i, 1);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int i = 0; i < NLD; ++i) load_b(0, i, 2);
    __builtin_amdgcn_sched_barrier(0);
    wb_bf16x8 a[3];
    dx_split8(ring[0][0], ring[0][1], a);

    // One wave per SIMD has nobody to hide an LDS round trip, a store to LDS or the split's VALU work behind, so a K step is
    // laid out by hand, in regions the scheduler may not move code across:
    //   head     barrier | request group 0's B fragments
    //   group c  request group c + 1's fragments | group c's MFMAs, and in their gaps: a third of the NEXT step's A split
    //            (groups 0 .. 2), one or two chunks of the stage of step s + 1 registers -> LDS buffer (s + 1) & 1 (free since
    //            the barrier), the same registers refilled with the stage of step s + 3, and (group 0) the ring slot that
    //            was split during the last step
    // Vector memory loads return in order and are waited for counting from the youngest.  Every K step issues the same loads
    // in the same order on every path (a wave whose tile is skipped multiplies zeros: no branch in the loop), so each wait
    // leaves a constant number of younger loads in flight: a stage chunk has two steps to arrive, an A fragment PD - 1.
    auto frags = [&](int buf, int ch, wb_bf16x8 (&b)[3][2]) {
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
#pragma unroll
            for (int j = ch * NT / NCH; j < (ch + 1) * NT / NCH; ++j) b[pl][j - ch * NT / NCH] = frag_b(buf, pl, j);
    };
    for (int s0 = 0; s0 < nk; s0 += PD) {
#pragma unroll
        for (int p = 0; p < PD; ++p) {
            const int s = s0 + p; // (s >= nk in the last round: zeros from A)
            wb_bf16x8 b[2][3][2], an[3];
            __syncthreads(); // buffer s & 1 is complete; nobody reads buffer (s + 1) & 1 any more
            frags(p & 1, 0, b[0]);
            __builtin_amdgcn_sched_barrier(0);
            wb_f32x4 v0 = __builtin_bit_cast(wb_f32x4, ring[(p + 1) % PD][0]), v1 = __builtin_bit_cast(wb_f32x4, ring[(p + 1) % PD][1]);
#pragma unroll
            for (int ch = 0; ch < NCH; ++ch) {
                if (ch + 1 < NCH) frags(p & 1, ch + 1, b[(ch + 1) & 1]);
#pragma unroll
                for (int t = 0; t < 6; ++t)
#pragma unroll
                    for (int j = ch * NT / NCH; j < (ch + 1) * NT / NCH; ++j)
                        acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[WB_TERM_A[t]], b[ch & 1][WB_TERM_B[t]][j - ch * NT / NCH], acc[j], 0, 0, 0);
                if (ch < 3) { // piece ch of the next step's A fragments: one step of wb_split4() per group, the two vectors side by side
                    const wb_u32x2 c0 = wb_pack(v0), c1 = wb_pack(v1);
                    an[ch] = __builtin_bit_cast(wb_bf16x8, wb_u32x4{c0[0], c0[1], c1[0], c1[1]});
                    if (ch < 2) { v0 -= wb_widen(c0); v1 -= wb_widen(c1); }
                }
                if (ch == 0) load_a(p, s + PD); // slot p held step s, split during step s - 1
#pragma unroll
                for (int i = ch * NLD / NCH; i < (ch + 1) * NLD / NCH; ++i) {
                    store_b((p + 1) & 1, i, (p + 1) & 1);
                    load_b((p + 1) & 1, i, s + 3);
                }
                __builtin_amdgcn_sched_group_barrier(0x100, 6, 0);
#pragma unroll
                for (int x = 0; x < 12; ++x) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                    __builtin_amdgcn_sched_group_barrier(0x002, 2, 0);
                    if (x % 4 == 1) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                    if (x % 4 == 3) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
                }
                __builtin_amdgcn_sched_barrier(0);
            }
#pragma unroll
            for (int pl = 0; pl < 3; ++pl) a[pl] = an[pl];
        }
    }

    // D[row = 4 lh + r][col = li] of column tile j
    if (active) {
#pragma unroll
        for (int j = 0; j < NT; ++j) {
            const int n = n0 + 16 * j + li;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int m = r0 + 4 * lh + r;
                if (m < g.M && n < g.N) g.out[(size_t)m * g.ldo + n] = acc[j][r];
            }
        }
    }
}

// one launch on stream st
template <int NT>
inline hipError_t dx0_split_launch_nt(hipStream_t st, const Dx0SplitArgs &g)
{
    static bool attr = false;
    constexpr int lds = dx0_split_lds_bytes();
    if (!attr) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_dx0_split<NT>, hipFuncAttributeMaxDynamicSharedMemorySize, lds);
        if (e != hipSuccess) return e;
        attr = true;
    }
    const dim3 grid((g.M + NVQA_DX_ROWS - 1) / NVQA_DX_ROWS, dx0_split_col_blocks(g.N));
    hipLaunchKernelGGL((k_dx0_split<NT>), grid, dim3(NVQA_DX_THREADS), lds, st, g);
    return hipGetLastError();
}
inline hipError_t dx0_split_launch(hipStream_t st, const Dx0SplitArgs &g)
{
    return dx0_split_nt(g.N) == 13 ? dx0_split_launch_nt<13>(st, g) : dx0_split_launch_nt<16>(st, g);
}

} // namespace nvqa
