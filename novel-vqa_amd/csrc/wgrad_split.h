// wgrad_split.h -- the time-batched weight gradients of the f32 mode as SIX bf16 MFMA terms per f32 product:
//     dW[M x N] = A^T B,   A = dG stored [K][lda] (K = steps x rows, M gate pre-activations contiguous),
//                          B = the layer's input / previous hidden state stored [K][ldb] (N contiguous)
// The three-way split of an f32 value, the six terms and their order, the k-major LDS image and the transposed fragment
// read are kmajor_bf16.h's.  What is this kernel's own:
//   * The split happens ONCE per value, on its way into LDS: three k-major bf16 images per operand.
//   * One LDS stage (6 images x 32 k x 256 B = 48 KB; with the stage list's tables the launch asks for 55 328 bytes)
//     and <= 256 registers: two workgroups share a CU, so one workgroup's fragment reads and barriers run under the
//     other's MFMAs.  Within a workgroup a K stage is
//         global loads of stage s+1 -> registers | fragments of stage s -> registers | barrier (LDS is free) |
//         96 MFMAs of stage s, with the split arithmetic and the LDS stores of stage s+1 in their gaps | barrier
//     (sched_group_barrier: 16 MFMAs alone while the loads land, then per MFMA three VALU instructions and per three
//     MFMAs one LDS store).  Loading two stages ahead (a second register set, 256 VGPRs) measured the same.
//   * Split-K over the slices into f32 slabs that the caller sums in z order.  The K stages that hold active rows
//     (ragged batches: rows >= nrows[step] of a step are zero padding; such stages are skipped when seg_rows % 32 == 0)
//     form one list, dealt to the slices round-robin: stage i of the list goes to slice i % (number of slices), so a
//     ragged batch loads every slice alike (ws_stage_list(), shared with k_wgrad_split2).  Rows between nrows[step] and
//     the end of their 32-row stage ARE multiplied: they must be zero in one operand and finite in the other, as for
//     gemm_big's K tiles.  Every workgroup builds its own list (a prefix sum over the steps and a search per stage, three
//     barriers): small beside the K loop.
#pragma once
#include "kmajor_bf16.h"

namespace nvqa {

struct WgradSplitArgs {
    const float *A, *B; // [K][lda], [K][ldb]
    float *out;         // slab z at out + z * slab_stride, [M][ldo]
    size_t slab_stride;
    const int *nrows;   // active rows per group of seg_rows K rows (NULL: all)
    int seg_rows;
    int lda, ldb, ldo, M, N, K; // M, N multiples of 4
};

#define NVQA_WS_BM 128
#define NVQA_WS_BN 128
#define NVQA_WS_BK 32
#define NVQA_WS_PLANE (NVQA_WS_BK * 256)
#define NVQA_WS_MAX_SEGS 256    // groups of K rows with a limit of their own (the tables hold MAX_SEGS + 1 prefix sums)
#define NVQA_WS_MAX_STAGES 1024 // K <= 32768
#define NVQA_WS_LDS_BYTES (6 * NVQA_WS_PLANE + 4 * (2 * (NVQA_WS_MAX_SEGS + 4) + NVQA_WS_MAX_STAGES))

// the shapes the kernel takes (the host falls back to the f32 chain otherwise)
inline bool wgrad_split_takes(int M, int N, int K, int lda, int ldb, int seg_rows)
{
    if (M % 4 || N % 4 || lda % 4 || ldb % 4 || K <= 0) return false;
    if ((K + NVQA_WS_BK - 1) / NVQA_WS_BK > NVQA_WS_MAX_STAGES) return false;
    if (seg_rows > 0 && seg_rows % NVQA_WS_BK == 0 && (K + seg_rows - 1) / seg_rows > NVQA_WS_MAX_SEGS) return false;
    return true;
}

// the K stages of slice z of ks: entry idx of the slice's list = stage z + idx ks of the list of active stages, its first
// K row in stage_k0[idx].  Returns the slice's number of stages.  Called by all THREADS threads of the workgroup; the
// tables (seg_cnt, seg_base: NVQA_WS_MAX_SEGS + 4 ints each, stage_k0: NVQA_WS_MAX_STAGES) are whole behind its last barrier.
template <int THREADS>
__device__ __forceinline__ int ws_stage_list(const WgradSplitArgs &g, int z, int ks, int *seg_cnt, int *seg_base, int *stage_k0)
{
    const int tid = threadIdx.x;
    const bool skip = g.nrows != nullptr && g.seg_rows > 0 && g.seg_rows % NVQA_WS_BK == 0;
    const int seg_rows = skip ? g.seg_rows : g.K, nseg = (g.K + seg_rows - 1) / seg_rows;
    // (strided over the block: nseg may equal the block size, and seg_base has nseg + 1 entries)
    for (int t = tid; t < nseg; t += THREADS) {
        int lim = min(seg_rows, g.K - t * seg_rows);
        if (skip) lim = min(lim, g.nrows[t]);
        seg_cnt[t] = lim > 0 ? (lim + NVQA_WS_BK - 1) / NVQA_WS_BK : 0;
    }
    __syncthreads();
    for (int t = tid; t <= nseg; t += THREADS) {
        int b = 0;
        for (int s = 0; s < t; ++s) b += seg_cnt[s];
        seg_base[t] = b;
    }
    __syncthreads();
    const int total = seg_base[nseg];
    const int nst = total > z ? (total - z + ks - 1) / ks : 0;
    for (int idx = tid; idx < nst; idx += THREADS) {
        const int i = z + idx * ks;
        int s = 0;
        while (seg_base[s + 1] <= i) ++s; // i < total = seg_base[nseg]
        stage_k0[idx] = s * seg_rows + NVQA_WS_BK * (i - seg_base[s]);
    }
    __syncthreads();
    return nst;
}

__global__ __launch_bounds__(256, 2) void k_wgrad_split(WgradSplitArgs g)
{
    extern __shared__ __attribute__((aligned(16))) unsigned char ws_smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lh = lane >> 4;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * NVQA_WS_BM, n0 = blockIdx.y * NVQA_WS_BN;
    const int z = blockIdx.z, kz = gridDim.z;
    unsigned char *As = ws_smem, *Bs = ws_smem + 3 * NVQA_WS_PLANE;
    int *seg_cnt = reinterpret_cast<int *>(ws_smem + 6 * NVQA_WS_PLANE), *seg_base = seg_cnt + NVQA_WS_MAX_SEGS + 4;
    int *stage_k0 = seg_base + NVQA_WS_MAX_SEGS + 4;

    const int nst = ws_stage_list<256>(g, z, kz, seg_cnt, seg_base, stage_k0);

    // staging: thread -> (row = tid / 32 + 8 i, 4 columns 4 (tid % 32) ..), i = 0 .. 3
    const int srow = tid >> 5, sc4 = tid & 31;
    const bool a_in = m0 + 4 * sc4 < g.M, b_in = n0 + 4 * sc4 < g.N;
    const float *pa = g.A + (size_t)srow * g.lda + m0 + 4 * sc4;
    const float *pb = g.B + (size_t)srow * g.ldb + n0 + 4 * sc4;
    wb_u32x4 ra[4], rb[4];
    auto load_stage = [&](int k0) { // k0 >= K: zeros
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const bool in = k0 + srow + 8 * i < g.K;
            ra[i] = a_in && in ? *reinterpret_cast<const wb_u32x4 *>(pa + (size_t)(k0 + 8 * i) * g.lda) : wb_u32x4{0, 0, 0, 0};
            rb[i] = b_in && in ? *reinterpret_cast<const wb_u32x4 *>(pb + (size_t)(k0 + 8 * i) * g.ldb) : wb_u32x4{0, 0, 0, 0};
        }
    };
    auto put = [&](unsigned char *img, int row, const wb_u32x4 &u) { // hi / mid / lo images of 4 values of one k row
        const unsigned o = wb_off(row, sc4 >> 1) + 8u * (sc4 & 1);
        wb_u32x2 h, m, l;
        wb_split4(__builtin_bit_cast(wb_f32x4, u), h, m, l);
        *reinterpret_cast<wb_u32x2 *>(img + o) = h;
        *reinterpret_cast<wb_u32x2 *>(img + NVQA_WS_PLANE + o) = m;
        *reinterpret_cast<wb_u32x2 *>(img + 2 * NVQA_WS_PLANE + o) = l;
    };
    auto store_stage = [&]() {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            put(As, srow + 8 * i, ra[i]);
            put(Bs, srow + 8 * i, rb[i]);
        }
    };
    // fragment of the 16 columns starting at c16 (tile-local), the stage's 32 k rows (kmajor_bf16.h)
    const int q = li >> 2, p = li & 3;
    auto frag = [&](const unsigned char *img, int c16) -> wb_bf16x8 {
        const int r0 = 8 * lh + q;
        const int ch = (c16 >> 3) + (p >> 1);
        return wb_frag((wb_lds_s16x4)(img + wb_off(r0, ch) + 8u * (p & 1)), (wb_lds_s16x4)(img + wb_off(r0 + 4, ch) + 8u * (p & 1)));
    };

    wb_f32x4 acc[4][4];
    wb_zero_tile(acc);

    if (nst > 0) {
        load_stage(stage_k0[0]);
        store_stage();
        __syncthreads();
        for (int st = 0; st < nst; ++st) {
            load_stage(st + 1 < nst ? stage_k0[st + 1] : g.K); // in flight under the fragment reads; past the end: zeros
            wb_bf16x8 a[3][4], b[3][4];                        // [hi, mid, lo]
#pragma unroll
            for (int pl = 0; pl < 3; ++pl)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    a[pl][i] = frag(As + pl * NVQA_WS_PLANE, wm * 64 + 16 * i);
                    b[pl][i] = frag(Bs + pl * NVQA_WS_PLANE, wn * 64 + 16 * i);
                }
            __syncthreads(); // every wave holds its fragments: the images may be overwritten
            // (nothing moves across: the split must not start -- and wait for the loads just issued -- above the fragment reads)
            __builtin_amdgcn_sched_barrier(0);
            // the six terms, smallest first (kmajor_bf16.h)
#pragma unroll
            for (int t = 0; t < 6; ++t)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[WB_TERM_A[t]][i], b[WB_TERM_B[t]][j], acc[i][j], 0, 0, 0);
            store_stage(); // the next stage's images (after the last stage: zeros nobody reads)
            // the split and the stores in the gaps of the MFMAs; the first 16 MFMAs alone: the loads are still landing
            __builtin_amdgcn_sched_group_barrier(0x008, 16, 0);
#pragma unroll
            for (int x = 0; x < 80; ++x) {
                __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);
                __builtin_amdgcn_sched_group_barrier(0x002, 3, 0);
                if (x % 3 == 2) __builtin_amdgcn_sched_group_barrier(0x200, 1, 0);
            }
            __syncthreads();
        }
    }
    wb_store_tile(g.out + (size_t)blockIdx.z * g.slab_stride, g.ldo, g.M, g.N, m0 + wm * 64, n0 + wn * 64, li, lh, acc);
}

// one launch on stream st: ks slices, slab z at g.out + z * g.slab_stride
inline hipError_t wgrad_split_launch(hipStream_t st, const WgradSplitArgs &g, int ks)
{
    static bool attr = false;
    if (!attr) {
        const hipError_t e = hipFuncSetAttribute((const void *)k_wgrad_split, hipFuncAttributeMaxDynamicSharedMemorySize, NVQA_WS_LDS_BYTES);
        if (e != hipSuccess) return e;
        attr = true;
    }
    const dim3 grid((g.M + NVQA_WS_BM - 1) / NVQA_WS_BM, (g.N + NVQA_WS_BN - 1) / NVQA_WS_BN, ks);
    hipLaunchKernelGGL(k_wgrad_split, grid, dim3(256), NVQA_WS_LDS_BYTES, st, g);
    return hipGetLastError();
}

} // namespace nvqa
