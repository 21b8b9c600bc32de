// wgrad_split2_check.hip -- TEST INFRASTRUCTURE (tests/test_gpu_wgrad_split2.py and tests/test_wgrad_split2_build.py, which
// compile it): k_wgrad_split2 (novel-vqa_amd/csrc/wgrad_split2.h) against k_wgrad_split (wgrad_split.h), both compiled into
// this program as the library compiles them.  Both kernels run on the same operands into NaN-prefilled slab buffers; all
// ks slabs must be equal AS BITS, no element of the new kernel's slabs may be left unwritten, and a second run of the new
// kernel must repeat its bits.  No tolerance: the old kernel is held against the f64 product by wgrad_split_check.hip.
// Operands as there: dG log-normal x 1e-3, the other operand 2 tanh x Bernoulli(0.5); ragged cases: rows >= nrows[step]
// are zero in dG and keep their (finite, non-zero) values in the other operand.
// One line per case (bits=: the new kernel's slabs, kmajor_check_common.h); exit status 1 on a difference.  With --time: microseconds per launch of both kernels at the step's
// two shapes instead.  Built by the tests, or by hand from this directory:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include -o wgrad_split2_check wgrad_split2_check.hip
#include "kmajor_check_common.h"
#include "../../novel-vqa_amd/csrc/wgrad_split2.h"
using namespace nvqa;

// out[0] += words that differ, out[1] += words of b still at the prefill pattern
__global__ void k_diff(const unsigned *a, const unsigned *b, size_t n, unsigned *out)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    if (a[i] != b[i]) atomicAdd(out, 1u);
    if (b[i] == 0xffffffffu) atomicAdd(out + 1, 1u);
}

struct Case { int M, N, B, T, ks; std::vector<int> nrows; bool given; int pad_a, pad_b; };

int main(int argc, char **argv)
{
    const bool timing = argc > 1 && !strcmp(argv[1], "--time");
    const unsigned POOL = (1u << 20) + 7;
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> hA(POOL), hB(POOL);
    for (auto &v : hA) v = kc_lognormal(rng, nd);
    for (auto &v : hB) v = kc_tanh_bernoulli(rng, nd);
    float *pA, *pB;
    if (hipMalloc(&pA, POOL * 4) != hipSuccess) { printf("no device\n"); return 2; }
    CK(hipMalloc(&pB, POOL * 4));
    CK(hipMemcpy(pA, hA.data(), POOL * 4, hipMemcpyHostToDevice));
    CK(hipMemcpy(pB, hB.data(), POOL * 4, hipMemcpyHostToDevice));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

    auto full = [](int B, int T) { return std::vector<int>(T, B); };
    auto ragged = [](int B, int T) { // questions start late: step t has nrows[t] active rows, growing with t
        std::vector<int> r(T);
        for (int t = 0; t < T; ++t) r[t] = std::min(B, 40 + (B * (t + 1) * 3) / (2 * T));
        return r;
    };
    std::vector<Case> cases;
    if (!timing) {
        cases.push_back({256, 128, 64, 1, 1, full(64, 1), false, 0, 0});                        // one tile, two stages, direct write
        cases.push_back({260, 200, 96, 7, 8, full(96, 7), false, 0, 0});                        // partial tiles; slices of 3 and of 2 stages
        cases.push_back({2048, 512, 160, 1, 8, full(160, 1), false, 0, 0});                     // three slices without a stage
        cases.push_back({512, 132, 64, 9, 4, {0, 5, 64, 33, 0, 64, 1, 32, 64}, true, 0, 0});    // ragged, padding stages skipped
        cases.push_back({388, 68, 50, 5, 2, {50, 40, 50, 13, 50}, true, 0, 0});                 // K 250: 26-row tail, nrows given but no skipping
        {
            std::vector<int> r(NVQA_WS_MAX_SEGS);
            for (int t = 0; t < NVQA_WS_MAX_SEGS; ++t) r[t] = (t * 7) % 33;
            cases.push_back({256, 200, 32, NVQA_WS_MAX_SEGS, 8, r, true, 0, 0});                // 256 steps of 32 rows, some empty
        }
        cases.push_back({300, 132, 64, 3, 2, full(64, 3), false, 64, 32});                      // lda = M + 64, ldb = N + 32
    }
    for (int N : {512, 200})
        for (int B : {512, 500})
            for (int ks : {8, 16})
                for (int rg = 0; rg < 2; ++rg) {
                    if (timing && (B != 512 || rg || ks != (N == 512 ? 8 : 16))) continue;
                    cases.push_back({2048, N, B, 26, ks, rg ? ragged(B, 26) : full(B, 26), rg != 0, 0, 0});
                }

    int bad = 0;
    for (const Case &cs : cases) {
        const int M = cs.M, N = cs.N, B = cs.B, T = cs.T, K = T * B, lda = M + cs.pad_a, ldb = N + cs.pad_b, ks = cs.ks;
        if (!wgrad_split_takes(M, N, K, lda, ldb, B) || !wgrad_split2_takes(M, N, K, lda, ldb, B)) { printf("shape not taken\n"); return 3; }
        const size_t mn = (size_t)M * N, words = mn * ks;
        float *dA, *dB, *dS1, *dS2, *dS3;
        int *dNr;
        unsigned *dCnt;
        CK(hipMalloc(&dA, (size_t)K * lda * 4));
        CK(hipMalloc(&dB, (size_t)K * ldb * 4));
        CK(hipMalloc(&dS1, words * 4)); CK(hipMalloc(&dS2, words * 4)); CK(hipMalloc(&dS3, words * 4));
        CK(hipMalloc(&dNr, T * 4));
        CK(hipMalloc(&dCnt, 4 * 4));
        CK(hipMemcpy(dNr, cs.nrows.data(), T * 4, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_fill, dim3(((size_t)K * lda + 255) / 256), dim3(256), 0, 0, dA, K, lda, M, pA, POOL, dNr, B, 1);
        hipLaunchKernelGGL(k_fill, dim3(((size_t)K * ldb + 255) / 256), dim3(256), 0, 0, dB, K, ldb, N, pB, POOL, dNr, B, 0);
        CK(hipMemset(dS1, 0xff, words * 4)); CK(hipMemset(dS2, 0xff, words * 4)); CK(hipMemset(dS3, 0xff, words * 4)); // NaNs
        CK(hipMemset(dCnt, 0, 4 * 4));
        const int *nr = cs.given ? dNr : nullptr;
        WgradSplitArgs g1{dA, dB, dS1, ks == 1 ? 0 : mn, nr, B, lda, ldb, N, M, N, K}, g2 = g1, g3 = g1;
        g2.out = dS2; g3.out = dS3;
        if (!timing) {
            CK(wgrad_split_launch(0, g1, ks));
            CK(wgrad_split2_launch(0, g2, ks));
            CK(wgrad_split2_launch(0, g3, ks));
            hipLaunchKernelGGL(k_diff, dim3((words + 255) / 256), dim3(256), 0, 0, (const unsigned *)dS1, (const unsigned *)dS2, words, dCnt);
            hipLaunchKernelGGL(k_diff, dim3((words + 255) / 256), dim3(256), 0, 0, (const unsigned *)dS2, (const unsigned *)dS3, words, dCnt + 2);
            CK(hipGetLastError());
            unsigned cnt[4];
            CK(hipMemcpy(cnt, dCnt, sizeof cnt, hipMemcpyDeviceToHost));
            std::vector<unsigned> slabs(words); // the new kernel's
            CK(hipMemcpy(slabs.data(), dS2, words * 4, hipMemcpyDeviceToHost));
            const bool ok = cnt[0] == 0 && cnt[1] == 0 && cnt[2] == 0;
            bad += ok ? 0 : 1;
            printf("M=%d N=%d K=%d (%d x %d) splitK=%d nrows=%s lda=%d ldb=%d: slabs %s (%u of %zu words differ), unwritten %u, rerun %s bits=%016llx %s\n",
                   M, N, K, T, B, ks, !cs.given ? "none" : "given", lda, ldb, cnt[0] ? "DIFFER" : "identical", cnt[0], words, cnt[1],
                   cnt[2] ? "DIFFERS" : "identical", (unsigned long long)kc_fnv1a(slabs.data(), words), ok ? "OK" : "MISS");
        } else {
            float us[2];
            for (int which = 0; which < 2; ++which) {
                auto launch = [&]() { return which == 0 ? wgrad_split_launch(0, g1, ks) : wgrad_split2_launch(0, g2, ks); };
                for (int i = 0; i < 3; ++i) CK(launch());
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < 20; ++i) CK(launch());
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                us[which] = ms * 50.f;
            }
            printf("time M=%d N=%d K=%d splitK=%d: k_wgrad_split %.1f us, k_wgrad_split2 %.1f us per launch (%.1f TF of f32-equivalent products)\n",
                   M, N, K, ks, us[0], us[1], 2.0 * M * N * K / (us[1] * 1e-6) * 1e-12);
        }
        fflush(stdout);
        CK(hipFree(dA)); CK(hipFree(dB)); CK(hipFree(dS1)); CK(hipFree(dS2)); CK(hipFree(dS3)); CK(hipFree(dNr)); CK(hipFree(dCnt));
    }
    return bad ? 1 : 0;
}
