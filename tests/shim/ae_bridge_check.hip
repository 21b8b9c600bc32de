// ae_bridge_check.hip -- TEST INFRASTRUCTURE (tests/test_gpu_ae_bridge.py, which compiles it): the forward of the arch1
// weak-paired auto-encoder's state bridge (novel-vqa_amd/csrc/ae_bridge.h, compiled into this program as the library compiles
// it) at the reference's shapes, B = 16 and B = 10 rows against W_q [1024 x 1024] and W_v [1024 x 4096] (and I = 2048), in two
// forms that share the finisher k_ae1wp_bridge_fwd:
//   split : k_ae1wp_bridge_gemv, ONE split-K launch over both products with the K slice of ae1wp_bridge_plan, into slabs;
//   wide  : the un-split form, two launches of the library's 128 x 128 LDS-tiled GEMM with K in one slice (one slab each).
// Both are held to an f64 evaluation on the host of the same sums (qc, ic and the decoder's initial state, each within 2e-5 of
// its largest element, the bound the step's tests put on every tensor), and a second run must give the same bits.
// One line per shape; exit status 1 on a miss.  With --time: both forms are timed in one process, alternating, in blocks of 50
// forwards (projections + finisher); median and range of the blocks in microseconds per forward.  Built by the test, or by
// hand from this directory:
//     hipcc -O3 -std=c++17 --offload-arch=gfx950 -I../../include -o ae_bridge_check ae_bridge_check.hip
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <random>
#include <vector>
#include "../../novel-vqa_amd/csrc/ae_bridge.h"
using namespace nvqa;

#define CK(x)                                                                                 \
    do {                                                                                      \
        hipError_t e_ = (x);                                                                  \
        if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 3; }    \
    } while (0)

typedef Cfg<16, 128, 128, 32, 4, 2, 1, 1> CfgWide; // = ae.hip's AeCfgWide

struct Bufs {
    float *qd, *vd, *wq, *wv, *bq, *bv, *j, *slabs, *qc, *ic, *c0, *h0;
};

static int run_split(hipStream_t s, const Bufs &d, const BridgePlan &pl, int B, int R, int I, const Drop &dr)
{
    const int N = 2 * R;
    BridgeGemvArgs g = {};
    g.x[0] = d.qd; g.x[1] = d.vd; g.w[0] = d.wq; g.w[1] = d.wv;
    g.slab[0] = d.slabs; g.slab[1] = d.slabs + (size_t)pl.zq * B * N;
    g.K[0] = N; g.K[1] = I; g.Z[0] = pl.zq; g.Z[1] = pl.zv; g.B = B; g.N = N; g.ks = pl.ks;
    hipLaunchKernelGGL(k_ae1wp_bridge_gemv, dim3(pl.workgroups), dim3(256), 0, s, g);
    hipLaunchKernelGGL(k_ae1wp_bridge_fwd, dim3((B * N + 255) / 256), dim3(256), 0, s, (const float *)g.slab[0], pl.zq,
                       (const float *)g.slab[1], pl.zv, B, R, (const float *)d.bq, (const float *)d.bv, (const float *)d.j, dr, d.qc,
                       d.ic, d.c0, d.h0);
    return 0;
}

static int run_wide(hipStream_t s, const Bufs &d, int B, int R, int I, const Drop &dr)
{
    const int N = 2 * R;
    GemmArgs gq = {}, gv = {};
    gq.xcd = 1; gq.A = d.qd; gq.B = d.wq; gq.lda = N; gq.ldb = N; gq.M = B; gq.N = N; gq.K = N; gq.kslice = N;
    gv.xcd = 1; gv.A = d.vd; gv.B = d.wv; gv.lda = I; gv.ldb = I; gv.M = B; gv.N = N; gv.K = I; gv.kslice = I;
    float *sq = d.slabs, *sv = d.slabs + (size_t)B * N;
    const EpiStore eq{sq, N, (size_t)B * N}, ev{sv, N, (size_t)B * N};
    (void)launch_gemm<CfgWide, A_KC, B_KC, false, EpiStore, 0>(s, gq, eq);
    (void)launch_gemm<CfgWide, A_KC, B_KC, false, EpiStore, 0>(s, gv, ev);
    hipLaunchKernelGGL(k_ae1wp_bridge_fwd, dim3((B * N + 255) / 256), dim3(256), 0, s, (const float *)sq, 1, (const float *)sv, 1, B, R,
                       (const float *)d.bq, (const float *)d.bv, (const float *)d.j, dr, d.qc, d.ic, d.c0, d.h0);
    return 0;
}

static double max_rel(const std::vector<float> &c, const std::vector<double> &ref)
{
    double dm = 0, rm = 0;
    for (size_t i = 0; i < ref.size(); ++i) {
        const double e = (double)c[i] - ref[i];
        if (!(e == e)) return 1e30;
        dm = fmax(dm, fabs(e)); rm = fmax(rm, fabs(ref[i]));
    }
    return dm / rm;
}

int main(int argc, char **argv)
{
    const bool timing = argc > 1 && !strcmp(argv[1], "--time");
    const int R = 512, N = 2 * R, IMAX = 4096, BMAX = 16;
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, 0) != hipSuccess || cus < 1) { printf("no device\n"); return 2; }
    std::mt19937 rng(1);
    std::uniform_real_distribution<float> u(-1.f, 1.f);
    // nn.Linear's default range for the weights; j like an LSTM state; vd = Dropout(L2-normalised post-ReLU features)
    std::vector<float> hwq((size_t)N * N), hwv((size_t)N * IMAX), hbq(N), hbv(N), hj((size_t)BMAX * N), hqd((size_t)BMAX * N),
        hvd((size_t)BMAX * IMAX);
    for (auto &v : hwq) v = u(rng) / sqrtf((float)N);
    for (auto &v : hbq) v = u(rng) / sqrtf((float)N);
    for (auto &v : hj) v = 0.8f * u(rng);
    for (size_t i = 0; i < hqd.size(); ++i) hqd[i] = (rng() & 1u) ? 2.f * hj[i] : 0.f;
    Bufs d;
    CK(hipMalloc(&d.qd, hqd.size() * 4)); CK(hipMalloc(&d.vd, hvd.size() * 4));
    CK(hipMalloc(&d.wq, hwq.size() * 4)); CK(hipMalloc(&d.wv, hwv.size() * 4));
    CK(hipMalloc(&d.bq, N * 4)); CK(hipMalloc(&d.bv, N * 4)); CK(hipMalloc(&d.j, hj.size() * 4));
    CK(hipMalloc(&d.slabs, (size_t)128 * BMAX * N * 4));
    CK(hipMalloc(&d.qc, (size_t)BMAX * N * 4)); CK(hipMalloc(&d.ic, (size_t)BMAX * N * 4));
    CK(hipMalloc(&d.c0, (size_t)BMAX * R * 4)); CK(hipMalloc(&d.h0, (size_t)BMAX * R * 4));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
    Drop dr;
    dr.mode = 1; dr.p = 0.5f; dr.inv_keep = 2.f; dr.seed = 123; dr.step = 7;

    int bad = 0;
    struct Case { int B, I; };
    for (const Case cs : {Case{16, 4096}, Case{10, 2048}, Case{10, 4096}, Case{16, 2048}}) {
        const int B = cs.B, I = cs.I;
        for (auto &v : hwv) v = u(rng) / sqrtf((float)I);
        for (auto &v : hbv) v = u(rng) / sqrtf((float)I);
        for (int b = 0; b < B; ++b) {
            double s = 0;
            for (int k = 0; k < I; ++k) { float f = u(rng); f = f > -0.4f ? fabsf(f) : 0.f; hvd[(size_t)b * I + k] = f; s += (double)f * f; }
            for (int k = 0; k < I; ++k) hvd[(size_t)b * I + k] = (rng() & 1u) ? 2.f * (float)(hvd[(size_t)b * I + k] / sqrt(s)) : 0.f;
        }
        CK(hipMemcpy(d.qd, hqd.data(), (size_t)B * N * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.vd, hvd.data(), (size_t)B * I * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.wq, hwq.data(), hwq.size() * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.wv, hwv.data(), (size_t)N * I * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.bq, hbq.data(), N * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.bv, hbv.data(), N * 4, hipMemcpyHostToDevice));
        CK(hipMemcpy(d.j, hj.data(), (size_t)B * N * 4, hipMemcpyHostToDevice));
        const BridgePlan pl = ae1wp_bridge_plan(B, N, N, I, cus);
        if (!pl.skinny || pl.zq + pl.zv > 128) { printf("unexpected plan\n"); return 3; }
        // f64 on the host
        const size_t bn = (size_t)B * N;
        std::vector<double> rq(bn), ri(bn), rs(bn);
        for (int b = 0; b < B; ++b)
            for (int n = 0; n < N; ++n) {
                double q = hbq[n], v = hbv[n];
                for (int k = 0; k < N; ++k) q += (double)hqd[(size_t)b * N + k] * (double)hwq[(size_t)n * N + k];
                for (int k = 0; k < I; ++k) v += (double)hvd[(size_t)b * I + k] * (double)hwv[(size_t)n * I + k];
                const size_t i = (size_t)b * N + n;
                rq[i] = tanh(q); ri[i] = tanh(v);
                rs[i] = (double)hj[i] + (double)nvqa_dropout_scale(dr.seed, dr.step, NVQA_SITE_Z, i, dr.p, dr.inv_keep) * rq[i] * ri[i];
            }
        auto fetch = [&](std::vector<float> &qc, std::vector<float> &ic, std::vector<float> &st) {
            std::vector<float> c(B * R), h(B * R);
            qc.resize(bn); ic.resize(bn); st.resize(bn);
            if (hipMemcpy(qc.data(), d.qc, bn * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (hipMemcpy(ic.data(), d.ic, bn * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (hipMemcpy(c.data(), d.c0, (size_t)B * R * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            if (hipMemcpy(h.data(), d.h0, (size_t)B * R * 4, hipMemcpyDeviceToHost) != hipSuccess) return false;
            for (int b = 0; b < B; ++b)
                for (int n = 0; n < N; ++n) st[(size_t)b * N + n] = n < R ? c[(size_t)b * R + n] : h[(size_t)b * R + n - R];
            return true;
        };
        std::vector<float> q1, i1, s1, q2, i2, s2, qw, iw, sw;
        CK(hipMemset(d.slabs, 0xff, (size_t)128 * BMAX * N * 4)); // NaNs: an unwritten slab element shows
        run_split(0, d, pl, B, R, I, dr);
        if (!fetch(q1, i1, s1)) return 3;
        CK(hipMemset(d.slabs, 0xff, (size_t)128 * BMAX * N * 4));
        run_split(0, d, pl, B, R, I, dr);
        if (!fetch(q2, i2, s2)) return 3;
        CK(hipMemset(d.slabs, 0xff, (size_t)128 * BMAX * N * 4));
        run_wide(0, d, B, R, I, dr);
        if (!fetch(qw, iw, sw)) return 3;
        CK(hipGetLastError());
        const bool same = q1 == q2 && i1 == i2 && s1 == s2;
        const double es = fmax(fmax(max_rel(q1, rq), max_rel(i1, ri)), max_rel(s1, rs));
        const double ew = fmax(fmax(max_rel(qw, rq), max_rel(iw, ri)), max_rel(sw, rs));
        const bool ok = same && es < 2e-5 && ew < 2e-5;
        bad += ok ? 0 : 1;
        printf("B=%d I=%d: split K slice %d, %d + %d slabs, %d workgroups: max rel %.3g; wide un-split: max rel %.3g; rerun %s %s\n", B, I,
               pl.ks, pl.zq, pl.zv, pl.workgroups, es, ew, same ? "identical" : "DIFFERS", ok ? "OK" : "MISS");
        if (timing) {
            const int NBLK = 9, PER = 50;
            std::vector<float> ts, tw;
            for (int i = 0; i < 10; ++i) { run_split(0, d, pl, B, R, I, dr); run_wide(0, d, B, R, I, dr); }
            for (int blk = 0; blk < 2 * NBLK; ++blk) {
                const bool split = blk % 2 == 0;
                CK(hipEventRecord(e0, 0));
                for (int i = 0; i < PER; ++i) {
                    if (split) run_split(0, d, pl, B, R, I, dr);
                    else run_wide(0, d, B, R, I, dr);
                }
                CK(hipEventRecord(e1, 0));
                CK(hipEventSynchronize(e1));
                float ms = 0;
                CK(hipEventElapsedTime(&ms, e0, e1));
                (split ? ts : tw).push_back(ms * 1000.f / PER);
            }
            std::sort(ts.begin(), ts.end());
            std::sort(tw.begin(), tw.end());
            printf("  time B=%d I=%d: split median %.2f us (blocks %.2f .. %.2f), wide median %.2f us (blocks %.2f .. %.2f), %d blocks of %d each, alternating\n",
                   B, I, ts[NBLK / 2], ts.front(), ts.back(), tw[NBLK / 2], tw.front(), tw.back(), NBLK, PER);
        }
        fflush(stdout);
    }
    return bad ? 1 : 0;
}
