// dx0_split_check.hip -- TEST INFRASTRUCTURE (tests/test_gpu_dx0_split.py and tests/test_dx0_split_build.py, which compile
// it): k_dx0_split (novel-vqa_amd/csrc/dx0_split.h) as the library compiles it, alone.  Per case the kernel runs into a
// NaN-prefilled output, on operands shaped like the step's (dG log-normal x 1e-3, W uniform in +-0.08, the three images of
// W^T made by the library's own TransposeJob code), and is held against the f64 product of the UNROUNDED operands beside an
// f32 fmaf chain on the same operands: L2-relative error within 1.5 x and max-relative error within 4 x of the chain's
// (tests/test_dx0_split_numerics.py).  Every element of a row that must be written has to be written, every row of a skipped
// 16-row tile must still be NaN, and a second run must repeat the bits.
// One line per case (bits=: kmajor_check_common.h); exit status 1 on a miss.  With --time: microseconds per launch of the old
// f32 MFMA GEMM and of the kernel at the step's two shapes, the two taking turns -- steady state (five rounds of 10
// launches back to back per kernel: dG, 109 MB, may sit in the 256 MB Infinity Cache) and first pass (five rounds of one
// launch behind a 1 GiB memset that evicts dG: what the step sees).  Built by the tests, or by hand:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include -o dx0_split_check dx0_split_check.hip
#include <algorithm>
#include "kmajor_check_common.h"
#include "../../novel-vqa_amd/csrc/kernels.h"
#include "../../novel-vqa_amd/csrc/dx0_split.h"
using namespace nvqa;

typedef Cfg<16, 64, 32, 64, 4, 2, 1, 1> CfgNarrow; // the old route's configurations (nvqa_api.hip)
typedef Cfg<16, 128, 128, 32, 4, 2, 1, 1> CfgBig16;

__global__ __launch_bounds__(256) void k_images(TransposeJob tj)
{
    __shared__ float tt[32][33];
    transpose_to_bf16_block(tj, blockIdx.x, tt);
}

struct Case { int M, N, K, seg_rows; std::vector<int> nrows; int pad; const char *what; };

int main(int argc, char **argv)
{
    const bool timing = argc > 1 && !strcmp(argv[1], "--time");
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::uniform_real_distribution<float> ud(-0.08f, 0.08f);
    {
        void *probe;
        if (hipMalloc(&probe, 16) != hipSuccess) { printf("no device\n"); return 2; }
        CK(hipFree(probe));
    }
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

    std::vector<Case> cases;
    if (!timing) {
        cases.push_back({16, 16, 32, 0, {}, 0, "one tile, one K step"});
        cases.push_back({40, 200, 64, 0, {}, 0, "partial last row tile, half-filled 13th column tile"});
        cases.push_back({16, 8, 2048, 0, {}, 0, "narrow N, long K"});
        cases.push_back({70, 512, 96, 0, {}, 0, "two column blocks"});
        cases.push_back({192, 200, 64, 64, {64, 17, 0}, 0, "full, partly skipped and empty segments"});
        cases.push_back({100, 200, 64, 20, {20, 7, 0, 20, 3}, 0, "seg_rows no multiple of 16: nothing skipped"});
        cases.push_back({33, 200, 64, 0, {}, 4, "padded leading dimension"});
        cases.push_back({32, 260, 64, 0, {}, 0, "N in the second column block"});
        cases.push_back({63, 208, 160, 0, {}, 0, "M one under the workgroup height, 13 full column tiles, K steps past the ring"});
        cases.push_back({65, 256, 32, 0, {}, 0, "M one over the workgroup height, 16 column tiles"});
        cases.push_back({128, 204, 64, 32, {32, 16, 1, 0}, 0, "two segments per workgroup"});
        cases.push_back({384, 200, 64, 128, {128, 70, 16}, 0, "segments of two row blocks: row blocks rotated inside each segment"});
    } else {
        cases.push_back({13312, 200, 2048, 0, {}, 0, "arch1 step"});
        cases.push_back({14336, 512, 2048, 0, {}, 0, "arch2 step"});
    }

    int bad = 0;
    for (const Case &cs : cases) {
        const int M = cs.M, N = cs.N, K = cs.K, lda = K + cs.pad;
        if (!dx0_split_takes(M, N, K, lda)) { printf("shape not taken\n"); return 3; }
        std::vector<float> hA((size_t)M * lda), hW((size_t)K * N);
        for (int m = 0; m < M; ++m)
            for (int k = 0; k < lda; ++k) {
                const float v = kc_lognormal(rng, nd);
                hA[(size_t)m * lda + k] = k < K ? v : nanf(""); // the padding between rows is never read
            }
        for (auto &v : hW) v = ud(rng);
        float *dA, *dW, *dO[2];
        unsigned short *dW3;
        int *dNr = nullptr;
        const size_t mn = (size_t)M * N;
        CK(hipMalloc(&dA, hA.size() * 4)); CK(hipMalloc(&dW, hW.size() * 4)); CK(hipMalloc(&dW3, 3 * hW.size() * 2));
        CK(hipMalloc(&dO[0], mn * 4)); CK(hipMalloc(&dO[1], mn * 4));
        CK(hipMemcpy(dA, hA.data(), hA.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dW, hW.data(), hW.size() * 4, hipMemcpyHostToDevice));
        if (!cs.nrows.empty()) {
            CK(hipMalloc(&dNr, cs.nrows.size() * 4));
            CK(hipMemcpy(dNr, cs.nrows.data(), cs.nrows.size() * 4, hipMemcpyHostToDevice));
        }
        TransposeJob tj;
        tj.W = dW; tj.out = dW3; tj.out_mid = dW3 + hW.size(); tj.out_lo = dW3 + 2 * hW.size();
        tj.rows = K; tj.cols = N; tj.nblocks = ((N + 31) / 32) * ((K + 31) / 32);
        hipLaunchKernelGGL(k_images, dim3(tj.nblocks), dim3(256), 0, 0, tj);
        CK(hipGetLastError());
        Dx0SplitArgs g = {};
        g.A = dA; g.lda = lda; g.W3 = dW3; g.out = dO[0]; g.ldo = N; g.M = M; g.N = N; g.K = K;
        g.nrows = dNr; g.seg_rows = cs.seg_rows;

        if (timing) {
            GemmArgs og = {};
            og.xcd = 1; og.A = dA; og.lda = lda; og.B = dW; og.ldb = N; og.M = M; og.N = N; og.K = og.kslice = K;
            auto launch = [&](int which) -> hipError_t {
                if (which == 0) {
                    if (N <= 256) return launch_gemm<CfgNarrow, A_KC, B_NC, false, EpiStore>(0, og, EpiStore{dO[1], N, 0});
                    return launch_gemm<CfgBig16, A_KC, B_NC, false, EpiStore>(0, og, EpiStore{dO[1], N, 0});
                }
                return dx0_split_launch(0, g);
            };
            void *evict;
            const size_t evict_bytes = (size_t)1 << 30;
            CK(hipMalloc(&evict, evict_bytes));
            // steady state: 5 rounds, each taking the two kernels in turn, 10 launches back to back per turn (min - max of the
            // rounds); first pass: 5 rounds in turn, one launch behind the evicting memset (median)
            float lo[2] = {1e30f, 1e30f}, hi[2] = {0.f, 0.f}, fp[2][5], first[2];
            for (int which = 0; which < 2; ++which)
                for (int i = 0; i < 3; ++i) CK(launch(which));
            for (int round = 0; round < 5; ++round)
                for (int which = 0; which < 2; ++which) {
                    CK(hipEventRecord(e0, 0));
                    for (int i = 0; i < 10; ++i) CK(launch(which));
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    float ms = 0;
                    CK(hipEventElapsedTime(&ms, e0, e1));
                    lo[which] = std::min(lo[which], ms * 100.f); hi[which] = std::max(hi[which], ms * 100.f);
                }
            for (int rep = 0; rep < 5; ++rep)
                for (int which = 0; which < 2; ++which) {
                    CK(hipMemsetAsync(evict, rep, evict_bytes, 0));
                    CK(hipEventRecord(e0, 0));
                    CK(launch(which));
                    CK(hipEventRecord(e1, 0));
                    CK(hipEventSynchronize(e1));
                    CK(hipEventElapsedTime(&fp[which][rep], e0, e1));
                }
            for (int which = 0; which < 2; ++which) {
                std::sort(fp[which], fp[which] + 5);
                first[which] = fp[which][2] * 1000.f; // median
            }
            CK(hipFree(evict));
            printf("time M=%d N=%d K=%d: steady state (5 alternated rounds of 10 launches, min-max) old f32 GEMM %.1f-%.1f us, k_dx0_split %.1f-%.1f us; "
                   "first pass (median of 5) old %.1f us, k_dx0_split %.1f us\n", M, N, K, lo[0], hi[0], lo[1], hi[1], first[0], first[1]);
        } else {
            // which rows must be written, which must have been skipped (a whole 16-row tile at or beyond its segment's limit)
            const bool skip = dNr && cs.seg_rows > 0 && cs.seg_rows % 16 == 0;
            std::vector<int> must(M, 1), skipped(M, 0);
            if (skip)
                for (int m = 0; m < M; ++m) {
                    const int t0 = m / 16 * 16, lim = cs.nrows[t0 / cs.seg_rows];
                    must[m] = m % cs.seg_rows < lim;
                    skipped[m] = t0 % cs.seg_rows >= lim;
                }
            std::vector<double> ref(mn);
            std::vector<float> chain(mn);
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) {
                    double s = 0.0;
                    float c = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const float a = hA[(size_t)m * lda + k], w = hW[(size_t)k * N + n];
                        s += (double)a * (double)w;
                        c = fmaf(a, w, c);
                    }
                    ref[(size_t)m * N + n] = s;
                    chain[(size_t)m * N + n] = c;
                }
            std::vector<float> h[2] = {std::vector<float>(mn), std::vector<float>(mn)};
            for (int run = 0; run < 2; ++run) {
                CK(hipMemset(dO[run], 0xff, mn * 4)); // NaNs
                g.out = dO[run];
                CK(dx0_split_launch(0, g));
                CK(hipDeviceSynchronize());
                CK(hipMemcpy(h[run].data(), dO[run], mn * 4, hipMemcpyDeviceToHost));
            }
            size_t unwritten = 0, touched = 0, rerun = 0;
            double refmax = 0, d6max = 0, d32max = 0, d6sq = 0, d32sq = 0, refsq = 0;
            for (int m = 0; m < M; ++m)
                for (int n = 0; n < N; ++n) {
                    const size_t i = (size_t)m * N + n;
                    unsigned b0, b1;
                    memcpy(&b0, &h[0][i], 4); memcpy(&b1, &h[1][i], 4);
                    rerun += b0 != b1;
                    if (skipped[m]) touched += b0 != 0xffffffffu;
                    if (!must[m]) continue;
                    if (b0 == 0xffffffffu) { ++unwritten; continue; }
                    const double d6 = (double)h[0][i] - ref[i], d32 = (double)chain[i] - ref[i];
                    refmax = std::max(refmax, fabs(ref[i])); d6max = std::max(d6max, fabs(d6)); d32max = std::max(d32max, fabs(d32));
                    d6sq += d6 * d6; d32sq += d32 * d32; refsq += ref[i] * ref[i];
                }
            const double m6 = d6max / refmax, m32 = d32max / refmax, l6 = sqrt(d6sq / refsq), l32 = sqrt(d32sq / refsq);
            const bool ok = unwritten == 0 && touched == 0 && rerun == 0 && l6 <= 1.5 * l32 && m6 <= 4.0 * m32;
            bad += ok ? 0 : 1;
            printf("M=%d N=%d K=%d lda=%d seg_rows=%d nrows=%s %s (%s): six terms max %.3g L2 %.3g, f32 chain max %.3g L2 %.3g (%.2f x, %.2f x), "
                   "unwritten %zu, skipped rows touched %zu, rerun %s bits=%016llx %s\n", M, N, K, lda, cs.seg_rows, dNr ? "given" : "none",
                   "lds", cs.what, m6, l6, m32, l32, m6 / m32, l6 / l32, unwritten, touched,
                   rerun ? "DIFFERS" : "identical", (unsigned long long)kc_fnv1a(h[0].data(), mn), ok ? "OK" : "MISS");
        }
        fflush(stdout);
        CK(hipFree(dA)); CK(hipFree(dW)); CK(hipFree(dW3)); CK(hipFree(dO[0])); CK(hipFree(dO[1]));
        if (dNr) CK(hipFree(dNr));
    }
    return bad ? 1 : 0;
}
