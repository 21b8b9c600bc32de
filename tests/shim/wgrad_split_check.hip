// wgrad_split_check.hip -- TEST INFRASTRUCTURE (tests/test_gpu_wgrad_split.py, which compiles it): the six-term bf16 weight-
// gradient kernel of the f32 mode (novel-vqa_amd/csrc/wgrad_split.h, compiled into this program as the library compiles it)
// on the shapes of the step -- dW[2048 x N] = dG^T X, N = 512 / 200, K = 13312 (B = 512) / 13000 (B = 500), split-K 8 and 16,
// one ragged profile of active rows, and the largest step count the kernel's tables take (256 steps of 32 rows, some of
// them empty) -- against a DOUBLE-PRECISION product of the UNROUNDED f32 operands, beside a plain f32
// fmaf chain with the same split-K on the same operands.  What is measured is how v_mfma_f32_16x16x32_bf16 sums its 32
// products: the six-term form must stay within 1.5 x of the f32 chain's L2-relative and 4 x of its max-relative error
// (margins of tests/test_wgrad_split_numerics.py's emulation), and a second run must give the same bits.
// One line per configuration (bits=: kmajor_check_common.h); exit status 1 on a miss.  With --time: microseconds per launch as well.  Built by the test,
// or by hand from this directory:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include -o wgrad_split_check wgrad_split_check.hip
#include "kmajor_check_common.h"
#include "../../novel-vqa_amd/csrc/wgrad_split.h"
using namespace nvqa;

int main(int argc, char **argv)
{
    const bool timing = argc > 1 && !strcmp(argv[1], "--time");
    const int M = 2048, KMAX = 13312, NMAX = 512, TMAX = NVQA_WS_MAX_SEGS;
    // dG: log-normal x 1e-3; the other operand: 2 tanh x Bernoulli(0.5), like Dropout(h)
    std::mt19937 rng(1);
    std::normal_distribution<float> nd(0.f, 1.f);
    std::vector<float> hA((size_t)KMAX * M), hB((size_t)KMAX * NMAX);
    for (auto &v : hA) v = kc_lognormal(rng, nd);
    for (auto &v : hB) v = kc_tanh_bernoulli(rng, nd);
    float *dA, *dB, *dS, *dO;
    double *dR;
    int *dNr;
    if (hipMalloc(&dA, hA.size() * 4) != hipSuccess) { printf("no device\n"); return 2; }
    CK(hipMalloc(&dB, hB.size() * 4));
    CK(hipMalloc(&dS, (size_t)16 * M * NMAX * 4));
    CK(hipMalloc(&dO, (size_t)M * NMAX * 4));
    CK(hipMalloc(&dR, (size_t)M * NMAX * 8));
    CK(hipMalloc(&dNr, TMAX * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));

    struct Case { int N, B, ks; bool ragged; int T; };
    std::vector<Case> cases;
    for (int N : {512, 200})
        for (int B : {512, 500})
            for (int ks : {8, 16}) cases.push_back({N, B, ks, false, 26});
    cases.push_back({512, 512, 8, true, 26});
    cases.push_back({200, 512, 16, true, 26});
    cases.push_back({200, 32, 8, true, TMAX}); // as many steps as wgrad_split_takes() admits

    int bad = 0;
    for (const Case &cs : cases) {
        const int N = cs.N, B = cs.B, T = cs.T, K = T * B, lda = M, ldb = N;
        // ragged: questions start late, so step t has nrows[t] active rows, growing with t; the other rows are zero
        std::vector<int> nrows(T);
        // (the many-step case: 0 .. B rows, in no order)
        for (int t = 0; t < T; ++t) nrows[t] = !cs.ragged ? B : B < 64 ? (t * 7) % (B + 1) : std::min(B, 40 + (B * (t + 1) * 3) / (2 * T));
        std::vector<float> a((size_t)K * lda), b((size_t)K * ldb);
        for (int k = 0; k < K; ++k) {
            const bool on = k % B < nrows[k / B];
            for (int m = 0; m < M; ++m) a[(size_t)k * lda + m] = on ? hA[(size_t)k * M + m] : 0.f;
            for (int n = 0; n < N; ++n) b[(size_t)k * ldb + n] = on ? hB[(size_t)k * NMAX + n] : 0.f;
        }
        CK(hipMemcpy(dA, a.data(), a.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dB, b.data(), b.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(dNr, nrows.data(), T * 4, hipMemcpyHostToDevice));
        if (K > KMAX || !wgrad_split_takes(M, N, K, lda, ldb, B)) { printf("shape not taken\n"); return 3; }
        const size_t mn = (size_t)M * N;
        std::vector<double> ref(mn);
        hipLaunchKernelGGL(k_ref_f64, dim3((N + 63) / 64, M), dim3(64), 0, 0, dA, dB, lda, ldb, M, N, K, dR);
        CK(hipMemcpy(ref.data(), dR, mn * 8, hipMemcpyDeviceToHost));
        // the reference itself, on the host, for a sample of rows
        for (int r = 0; r < 4; ++r) {
            const int m = (r * 977 + 13) % M;
            std::vector<double> o(N, 0.0);
            for (int k = 0; k < K; ++k) {
                const double av = a[(size_t)k * lda + m];
                for (int n = 0; n < N; ++n) o[n] += av * (double)b[(size_t)k * ldb + n];
            }
            for (int n = 0; n < N; ++n)
                if (fabs(o[n] - ref[(size_t)m * N + n]) > 1e-12 * (fabs(o[n]) + 1e-6)) { printf("reference mismatch at (%d, %d)\n", m, n); return 3; }
        }
        // f32 chain
        const int kslice = (K + cs.ks - 1) / cs.ks;
        std::vector<float> c32(mn), c6(mn), c6b(mn);
        CK(hipMemset(dS, 0xff, (size_t)16 * M * NMAX * 4));
        hipLaunchKernelGGL(k_f32_chain, dim3((N + 63) / 64, M, cs.ks), dim3(64), 0, 0, dA, dB, lda, ldb, M, N, K, kslice, dS);
        hipLaunchKernelGGL(k_sum_slabs, dim3((mn + 255) / 256), dim3(256), 0, 0, dS, cs.ks, mn, dO);
        CK(hipMemcpy(c32.data(), dO, mn * 4, hipMemcpyDeviceToHost));
        // six terms, twice
        WgradSplitArgs g{dA, dB, dS, mn, dNr, B, lda, ldb, N, M, N, K};
        for (int run = 0; run < 2; ++run) {
            CK(hipMemset(dS, 0xff, (size_t)16 * M * NMAX * 4)); // NaNs: an unwritten slab element shows
            CK(wgrad_split_launch(0, g, cs.ks));
            hipLaunchKernelGGL(k_sum_slabs, dim3((mn + 255) / 256), dim3(256), 0, 0, dS, cs.ks, mn, dO);
            CK(hipMemcpy((run ? c6b : c6).data(), dO, mn * 4, hipMemcpyDeviceToHost));
        }
        const bool same = !memcmp(c6.data(), c6b.data(), mn * 4);
        double l32, m32, l6, m6;
        errors(c32, ref, &l32, &m32);
        errors(c6, ref, &l6, &m6);
        const bool ok = same && l6 <= 1.5 * l32 && m6 <= 4.0 * m32;
        bad += ok ? 0 : 1;
        printf("N=%d K=%d splitK=%d ragged=%d: six terms L2 %.3g max %.3g, f32 chain L2 %.3g max %.3g, ratio L2 %.3f max %.3f, rerun %s bits=%016llx %s\n",
               N, K, cs.ks, (int)cs.ragged, l6, m6, l32, m32, l6 / l32, m6 / m32, same ? "identical" : "DIFFERS", (unsigned long long)kc_fnv1a(c6.data(), mn), ok ? "OK" : "MISS");
        if (timing) {
            for (int i = 0; i < 3; ++i) CK(wgrad_split_launch(0, g, cs.ks));
            CK(hipEventRecord(e0, 0));
            for (int i = 0; i < 20; ++i) CK(wgrad_split_launch(0, g, cs.ks));
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms = 0;
            CK(hipEventElapsedTime(&ms, e0, e1));
            printf("  time: %.1f us per launch, %.1f TF of f32-equivalent products\n", ms * 50.f, 2.0 * M * N * K / (ms / 20 * 1e-3) * 1e-12);
        }
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
