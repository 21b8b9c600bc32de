// wgrad_split2.h -- the six-term weight gradients of wgrad_split.h (same arithmetic, BIT-IDENTICAL slabs) with a larger tile
// and a pipelined K loop:
//   * 256 (M) x 128 (N) x 32 (K) per stage, 512 threads = 8 waves as 4 x 2, each wave the 64 x 64 sub-tile of
//     k_wgrad_split (same fragments, same MFMAs, same epilogue).  The X / H tile is split once for twice the dG rows:
//     24 values per thread and stage instead of 32.  One workgroup per CU, two waves per SIMD, <= 256 registers.
//   * TWO LDS buffers of nine 8 KB images (dG: hi / mid / lo x two 128-column halves, X / H: hi / mid / lo; the image
//     layout is kmajor_bf16.h's wb_off()), 72 KB each, and ONE barrier per stage.  A stage is six phases of 16 MFMAs,
//     one per term; what else a phase does rides in the gaps of its MFMAs:
//         term 0  lo  hi   | fragments mid / mid of this stage; split + store rows 0, 1 of stage s+1, reload for s+2
//         term 1  mid mid  | fragments hi / lo of this stage;   split + store rows 2, 3 of stage s+1, reload for s+2
//         term 2  hi  lo   | split + store the X / H rows of stage s+1, reload for s+2
//         term 3  mid hi   | barrier: stage s+1's images are whole, nobody reads this stage's images any more
//         term 4  hi  mid  | fragments lo / hi of stage s+1 (term 0 of the next stage)
//         term 5  hi  hi   |
//     Every fragment is read one phase before its MFMAs, every global load a whole stage before its split (ONE register
//     set: a row's registers are reloaded for stage s+2 as soon as its split has left them).
//   * Global loads are buffer loads on a descriptor of the stage's 32 rows: rows past K and columns past M / N read as
//     zero in hardware, so the loop body has no branch.  The loop is NOT peeled: the last two iterations load through a
//     descriptor of no rows (k0 = K), and the last one still splits and stores that stage of zeros into the free buffer
//     and reads term-0 fragments from it that nobody uses.  That is one stage's VALU and LDS work in the gaps of MFMAs
//     that run anyway (of 52 stages per workgroup at the step's shapes), and the only user of the k0 = K descriptor.
//   * A linear grid, remapped so that all tiles of a K slice share an XCD (and its L2) when the slice count is a multiple
//     of 8: one slice per XCD at 8 slices, two at 16.  Each L2 then fetches an eighth of both operands, once.
// What keeps the bits of k_wgrad_split: stage i of the list of active stages goes to slice i % ks, a slice runs its stages
// in list order, and every output element takes each stage as the same six v_mfma_f32_16x16x32_bf16 terms in the same
// order into one accumulator.  tests/shim/wgrad_split2_check.hip compares the two kernels slab by slab.
#pragma once
#include <type_traits>
#include "wgrad_split.h"

namespace nvqa {

#define NVQA_WS2_BM 256
#define NVQA_WS2_BN 128
#define NVQA_WS2_THREADS 512
#define NVQA_WS2_BUF (9 * NVQA_WS_PLANE)
#define NVQA_WS2_LDS_BYTES (2 * NVQA_WS2_BUF + 4 * (2 * (NVQA_WS_MAX_SEGS + 4) + NVQA_WS_MAX_STAGES))
#define NVQA_WS2_OOB 0x80000000u // a byte offset past every stage descriptor

// the shapes the kernel takes: k_wgrad_split's, with 32 rows of either operand inside a buffer descriptor's range
inline bool wgrad_split2_takes(int M, int N, int K, int lda, int ldb, int seg_rows)
{
    return wgrad_split_takes(M, N, K, lda, ldb, seg_rows) && lda <= (1 << 22) && ldb <= (1 << 22);
}

inline int wgrad_split2_blocks(int M, int N, int ks) { return ((M + NVQA_WS2_BM - 1) / NVQA_WS2_BM) * ((N + NVQA_WS2_BN - 1) / NVQA_WS2_BN) * ks; }

// grid: wgrad_split2_blocks(M, N, ks) x 1 x 1 (wgrad_split2_launch); slab z of the ks slabs at g.out + z * g.slab_stride
__global__ __launch_bounds__(NVQA_WS2_THREADS) void k_wgrad_split2(WgradSplitArgs g, int ks)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ws2_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lh = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    int *seg_cnt = reinterpret_cast<int *>(ws2_smem + 2 * NVQA_WS2_BUF), *seg_base = seg_cnt + NVQA_WS_MAX_SEGS + 4;
    int *stage_k0 = seg_base + NVQA_WS_MAX_SEGS + 4;

    // workgroup -> (slice, tile): blockIdx % 8 labels the workgroups that share an XCD
    const int tiles_m = (g.M + NVQA_WS2_BM - 1) / NVQA_WS2_BM, tiles = tiles_m * ((g.N + NVQA_WS2_BN - 1) / NVQA_WS2_BN);
    int z, tile;
    if (ks % 8 == 0) {
        const int per = ks / 8, local = blockIdx.x >> 3;
        z = (blockIdx.x & 7) * per + local / tiles;
        tile = local % tiles;
    } else {
        z = blockIdx.x / tiles;
        tile = blockIdx.x % tiles;
    }
    const int m0 = (tile % tiles_m) * NVQA_WS2_BM, n0 = (tile / tiles_m) * NVQA_WS2_BN;

    const int nst = ws_stage_list<NVQA_WS2_THREADS>(g, z, ks, seg_cnt, seg_base, stage_k0); // as k_wgrad_split builds it

    // staging: dG  thread -> (row = tid / 64 + 8 i, 4 columns 4 (tid % 64) ..), i = 0 .. 3
    //          X/H thread -> (row = tid / 32 + 16 i, 4 columns 4 (tid % 32) ..), i = 0, 1
    const int arow = tid >> 6, ac4 = tid & 63, asc4 = ac4 & 31, brow = tid >> 5, bsc4 = tid & 31;
    const bool a_in = m0 + 4 * ac4 < g.M, b_in = n0 + 4 * bsc4 < g.N;
    unsigned aoff[4], boff[2]; // byte offsets from the stage's first row
#pragma unroll
    for (int i = 0; i < 4; ++i) aoff[i] = a_in ? (unsigned)(((arow + 8 * i) * g.lda + m0 + 4 * ac4) * 4) : NVQA_WS2_OOB;
#pragma unroll
    for (int i = 0; i < 2; ++i) boff[i] = b_in ? (unsigned)(((brow + 16 * i) * g.ldb + n0 + 4 * bsc4) * 4) : NVQA_WS2_OOB;
    wb_u32x4 ra[4], rb[2];
    // descriptors of the 32 rows from k0 (k0 >= K: no rows, every load reads zeros); idx past the list: k0 = K
    auto stage_row = [&](int idx) { return __builtin_amdgcn_readfirstlane(idx < nst ? stage_k0[idx] : g.K); };
    auto rsrc = [&](const float *base, int ld, int k0) {
        const int rows = min(NVQA_WS_BK, g.K - k0);
        return __builtin_amdgcn_make_buffer_rsrc(const_cast<float *>(base + (size_t)k0 * ld), 0, rows * ld * 4, 0x00020000);
    };
    auto ldg = [](const __amdgpu_buffer_rsrc_t &r, unsigned off) { return __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0); };
    typedef __attribute__((address_space(3))) unsigned char *lds_t;
    // hi / mid / lo images (stride bytes apart) of 4 values of one k row
    auto put = [&](lds_t at, unsigned stride, const wb_u32x4 &u) {
        wb_u32x2 h, m, l;
        wb_split4(__builtin_bit_cast(wb_f32x4, u), h, m, l);
        *reinterpret_cast<__attribute__((address_space(3))) wb_u32x2 *>(at) = h;
        *reinterpret_cast<__attribute__((address_space(3))) wb_u32x2 *>(at + stride) = m;
        *reinterpret_cast<__attribute__((address_space(3))) wb_u32x2 *>(at + 2 * stride) = l;
    };
    // a buffer: dG plane pl, half h at (2 pl + h) planes, X / H plane pl at (6 + pl) planes.  Every LDS address of the
    // loop lives in a register that is moved to the other buffer once per stage: the stores start in buffer 1, the
    // fragment reads in buffer 0
    const lds_t smem = (lds_t)ws2_smem;
    lds_t wa[4], wb[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) wa[i] = smem + NVQA_WS2_BUF + (ac4 >> 5) * NVQA_WS_PLANE + wb_off(arow + 8 * i, asc4 >> 1) + 8u * (asc4 & 1);
#pragma unroll
    for (int i = 0; i < 2; ++i) wb[i] = smem + NVQA_WS2_BUF + 6 * NVQA_WS_PLANE + wb_off(brow + 16 * i, bsc4 >> 1) + 8u * (bsc4 & 1);
    auto put_a = [&](int i) { put(wa[i], 2 * NVQA_WS_PLANE, ra[i]); };
    auto put_b = [&](int i) { put(wb[i], NVQA_WS_PLANE, rb[i]); };
    // fragment of 16 columns, the stage's 32 k rows (wgrad_split.h): lane (li, lh) reads rows 8 lh + q and + 4
    const int q = li >> 2, p = li & 3;
    lds_t fa[4][2], fb[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int r0 = 8 * lh + q + 4 * h;
            fa[i][h] = smem + (wm >> 1) * NVQA_WS_PLANE + wb_off(r0, (((wm & 1) * 64 + 16 * i) >> 3) + (p >> 1)) + 8u * (p & 1);
            fb[i][h] = smem + 6 * NVQA_WS_PLANE + wb_off(r0, ((wn * 64 + 16 * i) >> 3) + (p >> 1)) + 8u * (p & 1);
        }
    struct Frag4 { wb_bf16x8 f[4]; };
    auto frag = [&](lds_t p0, lds_t p1, unsigned off) { return wb_frag((wb_lds_s16x4)(p0 + off), (wb_lds_s16x4)(p1 + off)); };
    auto frags_a = [&](int pl) {
        Frag4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r.f[i] = frag(fa[i][0], fa[i][1], 2 * pl * NVQA_WS_PLANE);
        return r;
    };
    auto frags_b = [&](int pl) {
        Frag4 r;
#pragma unroll
        for (int j = 0; j < 4; ++j) r.f[j] = frag(fb[j][0], fb[j][1], pl * NVQA_WS_PLANE);
        return r;
    };
    int flip = NVQA_WS2_BUF;
    auto other_buffer = [&]() { // between the last fragment read of a stage and the first of the next
#pragma unroll
        for (int i = 0; i < 4; ++i) { fa[i][0] += flip; fa[i][1] += flip; fb[i][0] += flip; fb[i][1] += flip; wa[i] -= flip; }
        wb[0] -= flip; wb[1] -= flip;
        flip = -flip;
    };

    wb_f32x4 acc[4][4];
    // (spelled out, not wb_zero_tile(): through the helper this kernel compiles to 220 registers instead of 216 -- profiles/kmajor_shared_ab.json)
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = wb_f32x4{0.f, 0.f, 0.f, 0.f};
    auto term = [&](const Frag4 &a, const Frag4 &b) {
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a.f[i], b.f[j], acc[i][j], 0, 0, 0);
    };
    // a phase's schedule, per MFMA of its 16: one LDS read (reads), three VALU instructions of the split (stores) with
    // one LDS store per three MFMAs, and the phase's two global loads behind the 8th and the 16th MFMA
    auto phase_sched = [](auto reads, auto stores) {
#pragma unroll
        for (int x = 0; x < 16; ++x) {
            __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
            if (decltype(reads)::value) __builtin_amdgcn_sched_group_barrier(0x100, 1, 0);
            if (decltype(stores)::value) {
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                if (x % 3 == 2 || x == 15) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
                if (x == 7 || x == 15) __builtin_amdgcn_sched_group_barrier(0x020, 1, 0);
            }
        }
    };
    typedef std::integral_constant<bool, true> yes_t;
    typedef std::integral_constant<bool, false> no_t;
    // the phases below are hand-laid: term t multiplies piece WB_TERM_A[t] of dG by piece WB_TERM_B[t] of X / H (0 hi, 1 mid, 2 lo)
    static_assert(WB_TERM_A[0] == 2 && WB_TERM_B[0] == 0 && WB_TERM_A[1] == 1 && WB_TERM_B[1] == 1 && WB_TERM_A[2] == 0 && WB_TERM_B[2] == 2 &&
                      WB_TERM_A[3] == 1 && WB_TERM_B[3] == 0 && WB_TERM_A[4] == 0 && WB_TERM_B[4] == 1 && WB_TERM_A[5] == 0 && WB_TERM_B[5] == 0,
                  "k_wgrad_split2's phases run lo hi, mid mid, hi lo, mid hi, hi mid, hi hi");

    if (nst > 0) {
        {   // stage 0 into buffer 0, stage 1 on its way
            const int k0 = stage_row(0), k1 = stage_row(1);
            const __amdgpu_buffer_rsrc_t r_a = rsrc(g.A, g.lda, k0), r_b = rsrc(g.B, g.ldb, k0);
#pragma unroll
            for (int i = 0; i < 4; ++i) ra[i] = ldg(r_a, aoff[i]);
#pragma unroll
            for (int i = 0; i < 2; ++i) rb[i] = ldg(r_b, boff[i]);
            const __amdgpu_buffer_rsrc_t r_a1 = rsrc(g.A, g.lda, k1), r_b1 = rsrc(g.B, g.ldb, k1);
#pragma unroll
            for (int i = 0; i < 4; ++i) { put(wa[i] - NVQA_WS2_BUF, 2 * NVQA_WS_PLANE, ra[i]); ra[i] = ldg(r_a1, aoff[i]); }
#pragma unroll
            for (int i = 0; i < 2; ++i) { put(wb[i] - NVQA_WS2_BUF, NVQA_WS_PLANE, rb[i]); rb[i] = ldg(r_b1, boff[i]); }
        }
        __syncthreads();
        Frag4 a_lo = frags_a(2), b_hi = frags_b(0);
        for (int st = 0; st < nst; ++st) {
            const int k2 = stage_row(st + 2);
            const __amdgpu_buffer_rsrc_t r_a = rsrc(g.A, g.lda, k2), r_b = rsrc(g.B, g.ldb, k2);
            __builtin_amdgcn_sched_barrier(0);
            // term 0: lo hi
            const Frag4 a_mid = frags_a(1), b_mid = frags_b(1);
            put_a(0); ra[0] = ldg(r_a, aoff[0]);
            put_a(1); ra[1] = ldg(r_a, aoff[1]);
            term(a_lo, b_hi);
            phase_sched(yes_t{}, yes_t{});
            __builtin_amdgcn_sched_barrier(0);
            // term 1: mid mid
            const Frag4 a_hi = frags_a(0), b_lo = frags_b(2);
            put_a(2); ra[2] = ldg(r_a, aoff[2]);
            put_a(3); ra[3] = ldg(r_a, aoff[3]);
            term(a_mid, b_mid);
            phase_sched(yes_t{}, yes_t{});
            __builtin_amdgcn_sched_barrier(0);
            // term 2: hi lo
            put_b(0); rb[0] = ldg(r_b, boff[0]);
            put_b(1); rb[1] = ldg(r_b, boff[1]);
            term(a_hi, b_lo);
            phase_sched(no_t{}, yes_t{});
            __builtin_amdgcn_sched_barrier(0);
            // term 3: mid hi; then stage st+1's images are whole and this stage's are free
            term(a_mid, b_hi);
            other_buffer();
            __builtin_amdgcn_sched_barrier(0);
            __syncthreads();
            __builtin_amdgcn_sched_barrier(0);
            // term 4: hi mid
            const Frag4 na_lo = frags_a(2), nb_hi = frags_b(0); // after the last stage: zeros nobody uses
            term(a_hi, b_mid);
            phase_sched(yes_t{}, no_t{});
            __builtin_amdgcn_sched_barrier(0);
            // term 5: hi hi
            term(a_hi, b_hi);
            __builtin_amdgcn_sched_barrier(0);
            a_lo = na_lo;
            b_hi = nb_hi;
        }
    }
    wb_store_tile(g.out + (size_t)z * g.slab_stride, g.ldo, g.M, g.N, m0 + wm * 64, n0 + wn * 64, li, lh, acc);
}

// one launch on stream st: ks slices, slab z at g.out + z * g.slab_stride
inline hipError_t wgrad_split2_launch(hipStream_t st, const WgradSplitArgs &g, int ks)
{
    static bool attr = false;
    if (!attr) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_wgrad_split2, hipFuncAttributeMaxDynamicSharedMemorySize, NVQA_WS2_LDS_BYTES);
        if (e != hipSuccess) return e;
        attr = true;
    }
    hipLaunchKernelGGL(k_wgrad_split2, dim3(wgrad_split2_blocks(g.M, g.N, ks)), dim3(NVQA_WS2_THREADS), NVQA_WS2_LDS_BYTES, st, g, ks);
    return hipGetLastError();
}

} // namespace nvqa
