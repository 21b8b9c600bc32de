// ae.hip -- the text auto-encoder of the reference's first stage (NVQA_ARCH_AE1): training forward, LanguageModelCriterion,
// backward, evaluate-mode loss and greedy decoding, sampling / beam decoding with log-probabilities (nvqa_ae_sample*, kernels
// in ae_decode.h), and the fused clamp / weight-decay / Adam update (any context); the
// arch2 text and weak-paired auto-encoders (NVQA_ARCH_AE2, NVQA_ARCH_AE2_WP) run the same code, below.
//
// Reference: 001_train_autoencoder/001_train_arch1_text_autoencoder.lua (lossFun :212-245, update :349-362, log line
// :266-268, eval_split :148-194) with misc/AutoEncoder_text_nostart.lua (model :26-31, forward :215-343, backward :348-393,
// criterion :399-455, sample :134-210) and misc/optim_updates.lua:78-111 (adam).  The decoder module is the one whose
// signature the auto-encoder calls: 003_train_vqa_arch2/misc/LSTM_decoder.lua (001's copy has only lstm_conventional and no
// LogSoftMax).
//
// The chain of one step (te encoder steps, then tmax + 1 decoder steps) and the token each step is fed on every arch are laid out
// in ae_chain.h, which holds the integer rules of a step once for the kernels and the host paths.  The image-first-token
// auto-encoder (NVQA_ARCH_AE2) is misc/AutoEncoder.lua with 001_train_arch2_text_autoencoder.lua; the weak-paired one
// (NVQA_ARCH_AE2_WP: AE2's chain with two token streams, the projected features as the image row, a frozen lookup table) is
// misc/AutoEncoderNull.lua with 004_train_arch2_weakpaired_autoencoder_*.lua.
// Per layer, one array of states over the whole chain (slot 0 = the zero initial state, slot q+1 = after chain step q):
// the decoder's initial state IS the encoder's final slot, and in the backward pass the decoder's state gradient at its
// step 0 flows into the encoder's last step through the ordinary recurrent product, with the encoder's W_h2h replaced by
// the decoder's at the boundary.  Each layer runs its whole chain before the layer above it starts (the decoder of layer l
// needs the encoder of layer l only); the backward pass runs the layers top-down.
// The arch1 weak-paired auto-encoder (NVQA_ARCH_AE1_WP, misc/AutoEncoder_vqa_arch.lua with
// 004_train_arch1_weakpaired_autoencoder_*.lua; one layer) is AE1's chain with two token streams, a frozen lookup that runs
// without its Dropout, and the bridge of ae_bridge.h between the two LSTMs: the state arrays hold one slot more, decoder step s
// reads slot te + 1 + s and writes te + 2 + s, slot te + 1 = the bridge's output.  The backward pass stops the recurrent
// product behind decoder step 0, runs the bridge's backward there, and starts the encoder's last step from its dc_T / dh_T.
// With the encoder skipped (encoder_skip_flag = 1) te = 0, j is the caller's and the encoder's gradient segment is zeroed.
// Data parallel (AE1 / AE2 with nvqa_ae_comm_init): the criterion's kernels scale by a rank weight
// n_r world / N read from device memory (N = the ranks' summed criterion counts, exchanged under the forward pass), and the
// backward pass hands each bucket of the gradient to the communication stream as soon as it is final.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>

#include "ae_bridge.h"
#include "ae_chain.h"
#include "ae_decode.h"
#include "gemm_f32.h"
#include "nvqa_ctx.h"
#include "prof.h"
#include "wgrad_bf16.h"

using namespace nvqa;

// vgg.hip: the raw-image route of the extractor with the features left on the device (the weak-paired *_images steps)
struct nvqa_vgg;
int nvqa_vgg_check_raw(const nvqa_vgg *v, const char *fn, const uint8_t *images, int n, int S, int xoff, int yoff,
                       const nvqa_dropout *dr);
int nvqa_vgg_forward_raw_device(nvqa_vgg *v, const char *fn, const uint8_t *images, int n, int S, int xoff, int yoff,
                                const nvqa_dropout *dr, const float **feats_dev, hipStream_t *stream);
int nvqa_vgg_features_taken(nvqa_vgg *v, hipStream_t consumer);
int nvqa_vgg_train_check_device(const nvqa_vgg *v, const char *fn);
int nvqa_vgg_train_forward_raw_device(nvqa_vgg *v, const char *fn, const uint8_t *images, int n, int S, int xoff, int yoff,
                                      const nvqa_dropout *dr, const float **feats_dev, hipStream_t *stream);
int nvqa_vgg_backward_device(nvqa_vgg *v, const char *fn, const float *dfhat_dev, int n, hipStream_t producer);
void nvqa_vgg_where(const nvqa_vgg *v, int *device, int *F);

namespace nvqa {

// the body in front of a weak-paired step: where ae_upload takes the features from instead of the host
struct AeBody {
    nvqa_vgg *vgg;
    const char *fn;
    const uint8_t *images;
    int S, xoff, yoff;
    const nvqa_dropout *dr;
    bool finetune = false; // the training forward, and the body's backward behind the step
};

// one batch as an entry point hands it over: the fields it has, the rest zero.  A parameter record and nothing more.
struct AeBatch {
    int n;                     // valid rows (a training step: B, set by ae_step_impl)
    const int32_t *tokens;     // [n x D]
    const float *images;       // AE2: [n x E], NULL: zero image rows
    const float *feats;        // weak-paired: [n x I], NULL with body
    const int32_t *enc_tokens; // weak-paired: [n x D], NULL: the null sentence (AE1_WP with enc_state: the encoder is skipped)
    const float *enc_state;    // AE1_WP: [n x 2R]
    const AeBody *body;        // weak-paired: the extractor in front of the step, in place of feats
};

struct AeState {
    std::vector<void *> dev, pinned; // every hipMalloc / hipHostMalloc of this state but the corpus: ae_destroy's list
    int flags = 0;       // AE_CHAIN_* (ae_chain.h)
    bool ae2 = false;    // NVQA_ARCH_AE2 (and AE2_WP): image row and START in front of the encoder's tokens
    bool wp = false;     // NVQA_ARCH_AE2_WP: projected features as the image row, encoder tokens of their own, frozen lookup
    int D = 0, QM = 0;   // seq_length; chain steps the buffers hold (AE1 2 D + 1, AE2 2 D + 3)
    int ldl = 0;         // leading dimension of the logits (V + 1 rounded up to 4 floats; the padding columns stay zero)
    int tmax = 0;        // last step's tmax
    int ncount = 0;      // last step's criterion count n (ae_chain.h criterion_count over the valid rows)
    int te = 0;          // last step's encoder steps = the chain step of decoder step 0 (AE1 tmax, AE2 tmax + 2)
    int dstr = 0;        // the D of the dropout counter indices (AE1 D, AE2 D + 1: a step stride of D + 2, nvqa_rng.h)
    float *img = nullptr;       // AE2: [B x E] image rows of the current batch (device); NULL input -> img_live = false
    float *h_img = nullptr;     // AE2: pinned staging of the image rows
    bool img_live = false;
    int32_t *tok = nullptr;     // [B x D] tokens of the current batch (device)
    int32_t *nrows = nullptr;   // device int = B (every row of the chain is active)
    int32_t *cur = nullptr;     // [B] greedy decoding: token fed at the next decoder step
    int32_t *samples = nullptr; // [B x D] greedy decoding output
    // lookup gradient: distinct tokens, their chunk ranges, the chunks' row ranges, the rows (grouped by token, row order)
    int32_t *lk_tok = nullptr, *lk_tc = nullptr, *lk_start = nullptr, *lk_pos = nullptr;
    int32_t *h_lk = nullptr;    // pinned staging: {nu, nchunks, the four arrays above}
    float *lk_part = nullptr;   // [chunks][E] partial sums
    int32_t *h_tok = nullptr;   // pinned staging of the tokens
    float *X0 = nullptr;        // [QM B][E] lookup outputs (tanh), the layer-0 inputs
    float *Gt[NVQA_MAX_LAYERS] = {};  // [QM B][4R] activated gates (forward) / d(pre-activations) (backward)
    float *Hs[NVQA_MAX_LAYERS] = {};  // [(QM + 1) B][R]
    float *Cs[NVQA_MAX_LAYERS] = {};  // [(QM + 1) B][R]
    float *U[NVQA_MAX_LAYERS] = {};   // [QM B][R] Dropout(h of the layer below), l >= 1
    float *dX = nullptr;        // [QM B][max(E, R)] time-batched d(input)
    float *dHx = nullptr;       // [QM B][R] dL/dh from outside the recurrence (projection, layer above)
    float *dc = nullptr;        // [B][R] carried cell gradient
    float *Htd = nullptr;       // [(D + 1) B][R] Dropout(top h) of the decoder steps
    float *logits = nullptr;    // [(D + 1) B][ldl] logits, then d(logits) in place
    float *rowloss = nullptr;   // [(D + 1) B]
    float *loss = nullptr;      // device scalar
    float *h_loss = nullptr;    // pinned
    // data parallel (nvqa_ae_comm_init): dpw = {n_r, N, w_r = n_r world / N, 1.0f} on the device.  The
    // criterion's kernels read their rank weight through wcur: dpw + 3 (exactly 1) without a communicator and in evaluate mode,
    // dpw + 2 in a data-parallel step, where the communication stream writes it under the forward pass
    float *dpw = nullptr;
    const float *wcur = nullptr;
    bool dp_wait = false;       // this step's rank weight is still on its way: the compute stream waits in front of the softmax
    bool loss_global = false;   // the last loss is a data-parallel step's: the exchanged sum in h_dp_status[2]
    int32_t *etok = nullptr;    // AE2_WP: [B x D] encoder tokens of the current batch (device; 0 rows = the null sentence)
    int32_t *h_etok = nullptr;  // AE2_WP: pinned staging
    float *feat = nullptr;      // AE2_WP: [B x I] features, L2-normalised in place (f^, kept for dW_p)
    float *h_feat = nullptr;    // AE2_WP: pinned staging
    float *wp_x = nullptr, *wp_g = nullptr, *wp_m = nullptr, *wp_v = nullptr; // AE2_WP: [W_p (E x I) | b_p (E)], its gradient, Adam
    float *wp_vel = nullptr;    // AE2_WP: the projection's velocity of nvqa_ae_wp_projection_update(NVQA_OPT_SGDM), allocated on first use
    double *wp_part = nullptr;  // AE2_WP: per-workgroup statistics of nvqa_ae_wp_projection_adam / _update
    int64_t wp_t = 0;           // AE2_WP: the projection's Adam step counter
    hipEvent_t staged = nullptr; // AE2_WP: the last batch's host-to-device copies are done (the staging buffers are free)
    bool staged_rec = false;
    // NVQA_ARCH_AE1_WP
    bool bridge = false;        // the bridge of ae_bridge.h sits between the LSTMs; decoder state slots are shifted by one
    bool feats = false;         // wp || bridge: features, encoder tokens of their own, frozen lookup
    bool skip = false;          // the current step got enc_state instead of enc_tokens (te = 0)
    // the bf16 operand mode of AE1 / AE2 (nvqa_ae_set_precision)
    bool bf16 = false;          // both operands of every dense product rounded to bf16 (nearest even), f32 accumulate
    bool p16 = false;           // bf16 && R % 8 == 0: the projection group reads bf16 images (below) instead of rounding f32 operands
    int ld16 = 0;               // leading dimension of the vocabulary-wide images (V + 1 rounded up to 8 bf16; the padding stays zero)
    unsigned short *Htd16 = nullptr; // [(D + 1) B][R] image of Htd
    unsigned short *G16 = nullptr;   // [(D + 1) B][ld16] image of (softmax - onehot) / n (the f32 logits are kept as they are)
    unsigned short *Wp16 = nullptr;  // [V + 1][R] image of W_proj, made per step (the weights move)
    unsigned short *WpT16 = nullptr; // [R][ld16] its transpose: K-contiguous for dH_top
    float *rowlse = nullptr;         // [(D + 1) B] log-sum-exp of a logits row
    int32_t *rowtgt = nullptr;       // [(D + 1) B] its target column, -1 = none: db_proj sums the f32 (softmax - onehot) / n from these
    float inv_n = 0.f;               // the last criterion's 1 / n
    BridgePlan plan;
    float *jbuf = nullptr, *h_j = nullptr; // [B x 2R] j = [c_T | h_T] (device) and the pinned staging of enc_state
    float *qd = nullptr, *vd = nullptr, *qc = nullptr, *ic = nullptr; // [B x 2R], [B x I], [B x 2R] x 2
    float *dqp = nullptr, *dvp = nullptr, *dh0 = nullptr, *dfeat = nullptr; // [B x 2R] x 2, [B x R], [B x I]
    float *br_slabs = nullptr;  // [zq + zv][B][2R] split-K partials of the bridge's projections
    float *slabs = nullptr;     // split-K partials of the weight gradients
    size_t slab_floats = 0;
    float *colpart = nullptr;   // column-sum partials
    size_t colpart_floats = 0;
    // the resident corpus of AE1 / AE2 (nvqa_ae_corpus_load): tokens on the device, and per row on the host
    // what the launch plan of a step needs -- no step reads a token back
    int32_t *corpus = nullptr;         // [corpus_rows x D] (device)
    int64_t corpus_rows = 0;
    std::vector<uint16_t> row_last;    // 1 + the row's last non-null column (0: a null row): tmax of a batch = their max
    std::vector<uint16_t> row_cnt;     // the row's criterion count = its non-null tokens + 1
    int32_t *lk_hist = nullptr;        // [QM][V + 2] rows per (chain step, token) of the device index build, zeroed per step
    int32_t *lk_base = nullptr;        // [QM][V + 2] a token's rows in the chain steps before q
    int32_t *lk_tot = nullptr;         // [V + 2] a token's rows, then (k_ae_lk_scan) the token's first slot of lk_pos
    int32_t *lk_chb = nullptr;         // [V + 2] the token's first chunk
    int32_t *lk_cnt = nullptr;         // {nu, nch} of the device-built index
    bool lk_dev = false;               // the current step's index was built on the device: nu / nch are lk_cnt's, not h_lk's
    hipEvent_t step_ev = nullptr;      // data parallel: the compute stream's position at the start of a resident step
    int64_t routes[2] = {0, 0};        // training steps fed from host tokens / from the resident corpus (nvqa_ae_step_routes)
    // decoding (nvqa_ae_sample*; ae_decode.h), allocated on first use
    float *slp = nullptr;              // [B x D] log-probabilities of the emitted tokens
    float *bm_h[NVQA_MAX_LAYERS] = {}; // beam: [B][R] the state the next decoder step reads (the last step's, re-ordered)
    float *bm_c[NVQA_MAX_LAYERS] = {};
    int32_t *bm_bp = nullptr, *bm_tk = nullptr; // beam: [D][B] back-pointers (decoder rows) and tokens (0 behind END) per position
    float *bm_lp = nullptr;            // beam: [D][B] their log-probabilities
    float *bm_score = nullptr;         // beam: [B] the hypotheses' scores
    int32_t *bm_fin = nullptr;         // beam: [B] 1 = the hypothesis has emitted END
    float *bm_csc = nullptr, *bm_clp = nullptr; // beam: [B][NVQA_AE_BEAM_MAX] a row's best (score, log-prob, column)
    int32_t *bm_cc = nullptr;
};

// zeroed device memory, recorded in own (NULL: the caller frees it); zs: the zero fill runs on that stream instead of the null one
static int ae_alloc(std::vector<void *> *own, void **p, size_t bytes, hipStream_t zs = nullptr)
{
    bytes = std::max<size_t>(bytes, 16);
    NVQA_HIP(hipMalloc(p, bytes));
    if (own) own->push_back(*p);
    NVQA_HIP(zs ? hipMemsetAsync(*p, 0, bytes, zs) : hipMemset(*p, 0, bytes));
    return 0;
}
#define AE_ALLOC(ptr, count) NVQA_TRY(ae_alloc(&c->ae->dev, (void **)&(ptr), (size_t)(count) * sizeof(*(ptr))))
#define AE_PINNED(ptr, count)                                                                           \
    do {                                                                                                \
        NVQA_HIP(hipHostMalloc((void **)&(ptr), (size_t)(count) * sizeof(*(ptr)), hipHostMallocDefault)); \
        c->ae->pinned.push_back(ptr);                                                                   \
    } while (0)

static GemmArgs ae_args(const float *A, int lda, const float *B, int ldb, int M, int N, int K, int kslice = 0)
{
    GemmArgs g = {};
    g.xcd = 1;
    g.A = A; g.B = B; g.lda = lda; g.ldb = ldb; g.M = M; g.N = N; g.K = K;
    g.kslice = kslice > 0 ? kslice : (K > 0 ? K : 1);
    return g;
}

static Drop ae_drop(const nvqa_dropout *dr, bool train)
{
    Drop d;
    if (!train || !dr || dr->mode == 0) {
        d.mode = 0; d.p = 0.f; d.inv_keep = 1.f; d.seed = 0; d.step = 0;
    } else {
        d.mode = 1; d.p = dr->p; d.inv_keep = 1.0f / (1.0f - dr->p); d.seed = dr->seed; d.step = dr->step;
    }
    return d;
}

// ------------------------------------------------------------------------------------------------------------------
// kernels
// ------------------------------------------------------------------------------------------------------------------
// the counter index of the lookup Dropout at chain row (q, b): te = tmax on AE1, the one arch that draws it
__device__ __forceinline__ uint64_t ae_lk_idx(int b, int q, int te, int D, int E, int e, uint32_t *site)
{
    if (q < te) { *site = NVQA_SITE_AE_ENC_LK; return ((uint64_t)b * D + q) * E + e; }
    *site = NVQA_SITE_AE_DEC_LK;
    return ((uint64_t)b * (D + 1) + (q - te)) * E + e;
}

// LookupTable -> Dropout -> Tanh (AutoEncoder_text_nostart.lua:28-31) of chain_token, chain steps from q0 on: one workgroup per row
__global__ void k_ae_embed(AeChain ch, const int32_t *enc, const int32_t *dec, const int32_t *direct, int E, int q0, const float *Wlk,
                           Drop dr, float *X0)
{
    const int r = q0 * ch.B + blockIdx.x, q = r / ch.B, b = r % ch.B;
    const float *w = Wlk + (size_t)(chain_token(ch, enc, dec, direct, q, b) - 1) * E;
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        uint32_t site;
        const uint64_t idx = ae_lk_idx(b, q, ch.te, ch.D, E, e, &site);
        X0[(size_t)r * E + e] = tanhf(dr.scale(site, idx) * w[e]);
    }
}

// AE2 layer-0 input X0 of chain steps [q0, q0 + gridDim.x / B) in one pass (AutoEncoder.lua:258-291, :318-348): the image row
// (img; NULL: zeros) where chain_token has none, else its row of a plain nn.LookupTable (:28): no dropout, no tanh.  One
// workgroup per row.
__global__ void k_ae2_assemble(AeChain ch, const int32_t *enc, const int32_t *dec, const int32_t *direct, const float *img, int E,
                               int q0, const float *Wlk, float *X0)
{
    const int r = q0 * ch.B + blockIdx.x, q = r / ch.B, b = r % ch.B;
    const int v = chain_token(ch, enc, dec, direct, q, b);
    const float *w = v ? Wlk + (size_t)(v - 1) * E : (img ? img + (size_t)b * E : nullptr);
    for (int e = threadIdx.x; e < E; e += blockDim.x) X0[(size_t)r * E + e] = w ? w[e] : 0.f;
}

// inter-layer / top-h dropout (forward: out = scale * in; backward: the same scale on the gradient).
// kind 0: input of layer l >= 1 at chain rows [r0, r0 + n): src row r is the output of chain step r / B (slot + 1 is added
//         by the caller's pointer), site NVQA_SITE_AE_LSTM; kind 1: top h of decoder step s = row / B, site NVQA_SITE_AE_TOP.
// IMG (bf16 operand mode, kind 1): the result also goes out as a bf16 image, the projection products' operand.
template <bool IMG = false>
__global__ void k_ae_drop(const float *src, float *dst, size_t n, int R, int B, int D, int L, int l, int tmax, int r0, int kind,
                          Drop dr, unsigned short *dst16 = nullptr)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const int r = r0 + (int)(i / R), j = (int)(i % R), q = r / B, b = r % B;
        float s = 1.f;
        if (dr.mode) {
            if (kind == 0) {
                const int k = q < tmax ? 0 : 1, t = q < tmax ? q : q - tmax;
                s = dr.scale(NVQA_SITE_AE_LSTM, ((((uint64_t)k * L + l) * B + b) * (D + 1) + t) * R + j);
            } else {
                s = dr.scale(NVQA_SITE_AE_TOP, ((uint64_t)b * (D + 1) + q) * R + j);
            }
        }
        dst[i] = s * src[i];
        if constexpr (IMG) dst16[i] = __builtin_bit_cast(unsigned short, (__bf16)(s * src[i]));
    }
}

// d(Dropout(top h)) from the projection's d(input) product, into dHx at the decoder's chain rows
struct EpiAeTop {
    float *dst; // dHx + tmax * B * R
    int R, B, D;
    Drop dr;
    __device__ __forceinline__ void operator()(int, int m, int n, float v) const
    {
        const int s = m / B, b = m % B;
        dst[(size_t)m * R + n] = dr.scale(NVQA_SITE_AE_TOP, ((uint64_t)b * (D + 1) + s) * R + n) * v;
    }
};

// logits = x W^T + b into a padded row
struct EpiAeBias {
    float *C;
    int ldc;
    const float *b;
    __device__ __forceinline__ void operator()(int, int m, int n, float v) const { C[(size_t)m * ldc + n] = v + b[n]; }
};

__device__ __forceinline__ void ae_lse_combine(float &m, float &s, float m2, float s2)
{
    if (m2 == -INFINITY) return;
    if (m == -INFINITY) { m = m2; s = s2; return; }
    if (m2 > m) { s = s * expf(m - m2) + s2; m = m2; }
    else s += s2 * expf(m2 - m);
}

// LanguageModelCriterion (AutoEncoder_text_nostart.lua:416-450) over LogSoftMax (LSTM_decoder.lua of 003, :60-61):
// one workgroup per row (s, b) of the logits, its target criterion_target's.  Statistics with an online max / sum-exp (one read);
// target rows then get (softmax - onehot) / n in place, rows without a target zeros (grad != 0).  nvalid: rows b >= nvalid
// carry no loss (nvqa_ae_evaluate with n < B).  Row losses go to rowloss; their sum is taken by k_ae_loss in a fixed order.
// IMG (bf16 operand mode, grad != 0): the f32 logits stay as they are; (softmax - onehot) / n goes out rounded to bf16 into the
// image g16 [rows][ld16] (padding columns and rows without a target zero), and the row's log-sum-exp and target are kept for
// k_ae_colsum_dlogits_part, which sums the f32 values for db_proj.
template <bool IMG>
__global__ __launch_bounds__(256) void k_ae_softmax(float *logits, int ldl, int Vp1, const int32_t *tok, int B, int D, int nvalid,
                                                    float inv_n, const float *rank_w, int grad, float *rowloss,
                                                    unsigned short *g16, int ld16, float *rowlse, int32_t *rowtgt)
{
    __shared__ float sm[8], ss[8];
    __shared__ float sh_lse;
    const int row = blockIdx.x, s = row / B, b = row % B;
    float *x = logits + (size_t)row * ldl;
    const int tgt = b < nvalid ? criterion_target(tok + (size_t)b * D, s, D, Vp1 - 1) : -1;
    if (tgt < 0) {
        if (threadIdx.x == 0) rowloss[row] = 0.f;
        if constexpr (IMG) {
            if (threadIdx.x == 0) rowtgt[row] = -1;
            uint4 *y = reinterpret_cast<uint4 *>(g16 + (size_t)row * ld16);
            for (int i = threadIdx.x; i < ld16 / 8; i += blockDim.x) y[i] = make_uint4(0u, 0u, 0u, 0u);
            return;
        }
        if (grad) {
            float4 *x4 = reinterpret_cast<float4 *>(x);
            for (int i = threadIdx.x; i < ldl / 4; i += blockDim.x) x4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    float m = -INFINITY, sum = 0.f;
    const float4 *x4 = reinterpret_cast<const float4 *>(x);
    const int n4 = ldl / 4;
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        const float4 v = x4[i];
        const float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (4 * i + k >= Vp1) continue;
            if (e[k] > m) { sum = sum * expf(m - e[k]) + 1.f; m = e[k]; }
            else sum += expf(e[k] - m);
        }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(sum, o, 64);
        ae_lse_combine(m, sum, m2, s2);
    }
    const int w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    if ((threadIdx.x & 63) == 0) { sm[w] = m; ss[w] = sum; }
    __syncthreads();
    if (threadIdx.x == 0) {
        float M = sm[0], S = ss[0];
        for (int k = 1; k < nw; ++k) ae_lse_combine(M, S, sm[k], ss[k]);
        const float lse = M + logf(S);
        sh_lse = lse;
        rowloss[row] = lse - x[tgt];
        if constexpr (IMG) { rowlse[row] = lse; rowtgt[row] = tgt; }
    }
    __syncthreads();
    if (!grad) return;
    const float lse = sh_lse;
    const float rw = rank_w[0]; // data parallel: n_r world / N, so that the ranks' sum / world is the global batch's gradient; else 1
    if constexpr (IMG) {
        uint4 *y = reinterpret_cast<uint4 *>(g16 + (size_t)row * ld16);
        for (int i = threadIdx.x; i < ld16 / 8; i += blockDim.x) {
            float e[8];
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const float4 v = 8 * i + 4 * h < ldl ? x4[2 * i + h] : make_float4(0.f, 0.f, 0.f, 0.f);
                e[4 * h] = v.x; e[4 * h + 1] = v.y; e[4 * h + 2] = v.z; e[4 * h + 3] = v.w;
            }
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int c = 8 * i + k;
                e[k] = c < Vp1 ? (expf(e[k] - lse) - (c == tgt ? 1.f : 0.f)) * inv_n * rw : 0.f;
            }
            const u32x2 lo = __builtin_bit_cast(u32x2, pack_bf16(make_float4(e[0], e[1], e[2], e[3])));
            const u32x2 hi = __builtin_bit_cast(u32x2, pack_bf16(make_float4(e[4], e[5], e[6], e[7])));
            y[i] = make_uint4(lo[0], lo[1], hi[0], hi[1]);
        }
        return;
    }
    float4 *y4 = reinterpret_cast<float4 *>(x);
    for (int i = threadIdx.x; i < n4; i += blockDim.x) {
        const float4 v = y4[i];
        float e[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = 4 * i + k;
            e[k] = c < Vp1 ? (expf(e[k] - lse) - (c == tgt ? 1.f : 0.f)) * inv_n * rw : 0.f;
        }
        y4[i] = make_float4(e[0], e[1], e[2], e[3]);
    }
}

// sum of the row losses in a fixed order (256 strided partials, then a tree) / n, times the rank weight (1 but in a
// data-parallel step, where the ranks' sum / world is then the global batch's loss)
__global__ __launch_bounds__(256) void k_ae_loss(const float *rowloss, int nrows, float inv_n, const float *rank_w, float *out)
{
    __shared__ float sh[256];
    float s = 0.f;
    for (int i = threadIdx.x; i < nrows; i += 256) s += rowloss[i];
    sh[threadIdx.x] = s;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) sh[threadIdx.x] += sh[threadIdx.x + o];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[0] = sh[0] * inv_n * rank_w[0];
}

// data parallel: cnt = {n_r, N, w_r, 1}.  k_ae_set_count writes this rank's criterion count, k_ae_rank_weight forms
// w_r = n_r world / N behind the all-reduce of the count, both on the communication stream.  n_r world and N are whole numbers
// below 2^24, so ranks with equal counts get exactly 1.
__global__ void k_ae_set_count(float *cnt, float n) { cnt[0] = n; }
__global__ void k_ae_rank_weight(float *cnt, float world) { cnt[2] = cnt[0] * world / cnt[1]; }

// greedy decoding: argmax of one decoder step's logits (first maximum, as torch.max on the CPU), 1-based; recorded as the
// sample of step s - 1 (sample() records the token fed at t >= 2) and fed to the next step
__global__ __launch_bounds__(256) void k_ae_argmax(const float *logits, int ldl, int Vp1, int D, int s, int32_t *cur, int32_t *samples)
{
    __shared__ float bm[4];
    __shared__ int bi[4];
    const int b = blockIdx.x;
    const float *x = logits + (size_t)b * ldl;
    float m = -INFINITY;
    int am = 0x7fffffff;
    for (int c = threadIdx.x; c < Vp1; c += blockDim.x) {
        const float v = x[c];
        if (v > m) { m = v; am = c; }
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const float m2 = __shfl_xor(m, o, 64);
        const int a2 = __shfl_xor(am, o, 64);
        if (m2 > m || (m2 == m && a2 < am)) { m = m2; am = a2; }
    }
    if ((threadIdx.x & 63) == 0) { bm[threadIdx.x >> 6] = m; bi[threadIdx.x >> 6] = am; }
    __syncthreads();
    if (threadIdx.x == 0) {
        for (int k = 1; k < 4; ++k)
            if (bm[k] > m || (bm[k] == m && bi[k] < am)) { m = bm[k]; am = bi[k]; }
        cur[b] = am + 1;
        samples[(size_t)b * D + s] = am + 1;
    }
}

// column sums of X [M][ld] (first N columns), deterministic: stripes of rows -> part[S][N], then the S partials in order
__global__ void k_ae_colsum_part(const float *X, int M, int N, int ld, int rps, float *part)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int m0 = blockIdx.y * rps, m1 = min(M, m0 + rps);
    float s0 = 0.f, s1 = 0.f;
    int m = m0;
    for (; m + 1 < m1; m += 2) { s0 += X[(size_t)m * ld + n]; s1 += X[(size_t)(m + 1) * ld + n]; }
    if (m < m1) s0 += X[(size_t)m * ld + n];
    part[(size_t)blockIdx.y * N + n] = s0 + s1;
}
__global__ void k_ae_colsum_final(const float *part, int S, int N, float *out, float *out2)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    float s = 0.f;
    for (int i = 0; i < S; ++i) s += part[(size_t)i * N + n];
    out[n] = s;
    if (out2) out2[n] = s;
}

// bf16 operand mode: k_ae_colsum_part over d(logits) = (softmax - onehot) / n, formed here in f32 from the logits and the rows'
// log-sum-exp / target as k_ae_softmax forms it (only its bf16 image is stored): db_proj sums what the f32 path sums, in its order
__global__ void k_ae_colsum_dlogits_part(const float *X, const float *rowlse, const int32_t *rowtgt, float inv_n, const float *rank_w,
                                         int M, int N, int ld, int rps, float *part)
{
    const int n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    const int m0 = blockIdx.y * rps, m1 = min(M, m0 + rps);
    const float w = rank_w[0];
    auto val = [&](int m) {
        const int t = rowtgt[m];
        return t < 0 ? 0.f : (expf(X[(size_t)m * ld + n] - rowlse[m]) - (n == t ? 1.f : 0.f)) * inv_n * w;
    };
    float s0 = 0.f, s1 = 0.f;
    int m = m0;
    for (; m + 1 < m1; m += 2) { s0 += val(m); s1 += val(m + 1); }
    if (m < m1) s0 += val(m);
    part[(size_t)blockIdx.y * N + n] = s0 + s1;
}

// bf16 operand mode: the two bf16 images of W_proj [Vp1][R] (R % 8 == 0), one 64 x 64 tile per workgroup through LDS:
// W16 [Vp1][R] (K = R contiguous: the logits product) and WT16 [R][ld16] (K = V + 1 contiguous: dH_top), whose padding
// columns [Vp1, ld16) are written as zeros.  16-byte global loads and stores on both sides.
__global__ __launch_bounds__(256) void k_ae_wproj_images(const float *W, int Vp1, int R, int ld16, unsigned short *W16,
                                                         unsigned short *WT16)
{
    __shared__ unsigned t[64][33]; // [v][r pairs], an odd pitch in words
    const int v0 = blockIdx.x * 64, r0 = blockIdx.y * 64, tid = threadIdx.x;
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int vl = (tid >> 3) + 32 * ps, rl = 8 * (tid & 7), v = v0 + vl, r = r0 + rl;
        u32x2 lo = {0u, 0u}, hi = {0u, 0u};
        if (v < Vp1 && r < R) {
            const float4 *p = reinterpret_cast<const float4 *>(W + (size_t)v * R + r);
            lo = __builtin_bit_cast(u32x2, pack_bf16(p[0]));
            hi = __builtin_bit_cast(u32x2, pack_bf16(p[1]));
            *reinterpret_cast<uint4 *>(W16 + (size_t)v * R + r) = make_uint4(lo[0], lo[1], hi[0], hi[1]);
        }
        t[vl][rl / 2] = lo[0]; t[vl][rl / 2 + 1] = lo[1]; t[vl][rl / 2 + 2] = hi[0]; t[vl][rl / 2 + 3] = hi[1];
    }
    __syncthreads();
#pragma unroll
    for (int ps = 0; ps < 2; ++ps) {
        const int vq = tid & 7, rl = (tid >> 3) + 32 * ps, v = v0 + 8 * vq, r = r0 + rl;
        if (v >= ld16 || r >= R) continue;
        unsigned w[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const unsigned a = t[8 * vq + 2 * j][rl >> 1], b = t[8 * vq + 2 * j + 1][rl >> 1];
            const unsigned sh = 16 * (rl & 1);
            w[j] = ((a >> sh) & 0xffffu) | (((b >> sh) & 0xffffu) << 16);
        }
        *reinterpret_cast<uint4 *>(WT16 + (size_t)r * ld16 + v) = make_uint4(w[0], w[1], w[2], w[3]);
    }
}

// split-K slabs [Z][n] -> out[n], fixed order
__global__ void k_ae_slab_sum(const float *slabs, int Z, size_t n, float *out)
{
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        float s = 0.f;
        for (int z = 0; z < Z; ++z) s += slabs[(size_t)z * n + i];
        out[i] = s;
    }
}

// lookup-table gradient (LookupTable:backward of both clone sets, :366-367 / :385-386), deterministic in two passes: the rows
// of each distinct token (encoder and decoder positions, in row order) come in chunks of at most NVQA_AE_LK_CHUNK; pass 1
// sums each chunk through the backward of Tanh and Dropout, pass 2 adds a token's chunks in order.  (One workgroup per
// token summing all its rows serially took 13 ms at the default shape: the START token alone has B rows, the padding
// token 1 thousands.)  Rows of tokens absent from the batch were zeroed by the caller.
// cnt (the device-built index of a resident step): the launch's grid is an upper bound, workgroups past *cnt return
__global__ void k_ae_lk_part(const int32_t *lk_start, const int32_t *lk_pos, const float *X0, const float *dX, int B, int D,
                             int E, int tmax, Drop dr, float *part, const int32_t *cnt)
{
    if (cnt && (int)blockIdx.x >= cnt[0]) return;
    const int p0 = lk_start[blockIdx.x], p1 = lk_start[blockIdx.x + 1];
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        float s = 0.f;
        for (int p = p0; p < p1; ++p) {
            const int r = lk_pos[p], q = r / B, b = r % B;
            const float y = X0[(size_t)r * E + e];
            uint32_t site;
            const uint64_t idx = ae_lk_idx(b, q, tmax, D, E, e, &site);
            s += dX[(size_t)r * E + e] * (1.f - y * y) * dr.scale(site, idx);
        }
        part[(size_t)blockIdx.x * E + e] = s;
    }
}
// AE2 (plain LookupTable): pass 1 is the plain sum of the chunk's d(input) rows
__global__ void k_ae2_lk_part(const int32_t *lk_start, const int32_t *lk_pos, const float *dX, int E, float *part, const int32_t *cnt)
{
    if (cnt && (int)blockIdx.x >= cnt[0]) return;
    const int p0 = lk_start[blockIdx.x], p1 = lk_start[blockIdx.x + 1];
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        float s = 0.f;
        for (int p = p0; p < p1; ++p) s += dX[(size_t)lk_pos[p] * E + e];
        part[(size_t)blockIdx.x * E + e] = s;
    }
}
__global__ void k_ae_lk_sum(const int32_t *lk_tok, const int32_t *lk_tc, const float *part, int E, float *dW, const int32_t *cnt)
{
    if (cnt && (int)blockIdx.x >= cnt[0]) return;
    const int u = lk_tok[blockIdx.x], c0 = lk_tc[blockIdx.x], c1 = lk_tc[blockIdx.x + 1];
    for (int e = threadIdx.x; e < E; e += blockDim.x) {
        float s = 0.f;
        for (int k = c0; k < c1; ++k) s += part[(size_t)k * E + e];
        dW[(size_t)(u - 1) * E + e] = s;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The resident corpus (nvqa_ae_corpus_load / nvqa_ae_step_rows): the batch is gathered from the corpus in
// HBM by row ids that travel as kernel arguments, and the lookup gradient's index above is built here instead of on the host --
// the same four arrays, entry for entry, so the lookup gradient keeps its bits.
// ------------------------------------------------------------------------------------------------------------------
// tok rows [b0, b0 + nb) of the batch = corpus rows ids.q[0 .. nb), rows from n on zero (nvqa_ae_evaluate_rows with n < B)
__global__ void k_ae_gather_rows(const int32_t *corpus, QIdxArg ids, int b0, int nb, int n, int D, int32_t *tok)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nb * D) return;
    const int bl = i / D, t = i % D, b = b0 + bl;
    tok[(size_t)b * D + t] = b < n ? corpus[(size_t)ids.q[bl] * D + t] : 0;
}

// hist[q][v] = rows of chain step q that carry token v (W = V + 2 bins per step).  Integer counts: their order does not matter.
__global__ void k_ae_lk_hist(AeChain ch, const int32_t *tok, int r_lo, int np, int32_t *hist)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= np) return;
    const int r = r_lo + i, q = r / ch.B, b = r % ch.B;
    atomicAdd(hist + (size_t)q * (ch.V + 2) + chain_token(ch, tok, tok, nullptr, q, b), 1);
}

// per token: base[q][v] = its rows in the chain steps before q, tot[v] = all its rows.  One thread per token.
__global__ void k_ae_lk_prefix(const int32_t *__restrict__ hist, int V, int q_lo, int Q, int32_t *__restrict__ base,
                               int32_t *__restrict__ tot)
{
    const int v = 1 + blockIdx.x * blockDim.x + threadIdx.x, W = V + 2;
    if (v > V + 1) return;
    int run = 0;
    for (int q = q_lo; q < Q; ++q) {
        base[(size_t)q * W + v] = run;
        run += hist[(size_t)q * W + v];
    }
    tot[v] = run;
}

// exclusive scan of one int per thread over a workgroup of NT threads (wave64 shuffles, then the waves' totals through LDS)
template <int NT>
__device__ __forceinline__ int ae_block_excl_scan(int x, int *wsum, int *total)
{
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int inc = x;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const int y = __shfl_up(inc, o, 64);
        if (lane >= o) inc += y;
    }
    __syncthreads(); // (wsum may still be read from the previous scan)
    if (lane == 63) wsum[w] = inc;
    __syncthreads();
    int off = 0, tot = 0;
#pragma unroll
    for (int k = 0; k < NT / 64; ++k) {
        if (k < w) off += wsum[k];
        tot += wsum[k];
    }
    *total = tot;
    return off + inc - x;
}

// one workgroup over the V + 1 bins, each thread a run of consecutive tokens: the distinct tokens ascending (lk_tok), their first
// chunk (lk_tc, and chb[v] for k_ae_lk_rank), and tot[v] turned into the token's first slot of lk_pos; cnt = {nu, nch}, and the
// closing entries lk_tc[nu] = nch, lk_start[nch] = rows.  The chunks' starts themselves are written by k_ae_lk_rank.
#define NVQA_AE_SCAN_NT 1024
__global__ __launch_bounds__(NVQA_AE_SCAN_NT) void k_ae_lk_scan(int V, int32_t *tot, int32_t *chb, int32_t *lk_tok, int32_t *lk_tc,
                                                                int32_t *lk_start, int32_t *cnt)
{
    __shared__ int wsum[NVQA_AE_SCAN_NT / 64];
    const int nb = V + 1, per = (nb + NVQA_AE_SCAN_NT - 1) / NVQA_AE_SCAN_NT;
    const int v0 = 1 + (int)threadIdx.x * per, v1 = min(v0 + per, nb + 1);
    int nu = 0, nch = 0, acc = 0;
    for (int v = v0; v < v1; ++v) {
        const int n = tot[v];
        nu += n > 0 ? 1 : 0;
        nch += (n + NVQA_AE_LK_CHUNK - 1) / NVQA_AE_LK_CHUNK;
        acc += n;
    }
    int nu_all, nch_all, acc_all;
    int u = ae_block_excl_scan<NVQA_AE_SCAN_NT>(nu, wsum, &nu_all);
    int ch = ae_block_excl_scan<NVQA_AE_SCAN_NT>(nch, wsum, &nch_all);
    int at = ae_block_excl_scan<NVQA_AE_SCAN_NT>(acc, wsum, &acc_all);
    for (int v = v0; v < v1; ++v) {
        const int n = tot[v];
        if (n == 0) continue;
        lk_tok[u] = v;
        lk_tc[u] = ch;
        chb[v] = ch;
        tot[v] = at;
        ++u;
        ch += (n + NVQA_AE_LK_CHUNK - 1) / NVQA_AE_LK_CHUNK;
        at += n;
    }
    if (threadIdx.x == 0) {
        lk_tc[nu_all] = nch_all;
        lk_start[nch_all] = acc_all;
        cnt[0] = nu_all;
        cnt[1] = nch_all;
    }
}

// chain row (q, b) goes to slot first[v] + base[q][v] + (rows b' < b of step q with the same token): ascending chain rows inside
// a token, whatever the schedule.  Workgroup (q, block of 256 rows); the step's tokens pass through LDS 256 at a time.  A row
// that opens a chunk writes the chunk's start.
__global__ __launch_bounds__(256) void k_ae_lk_rank(AeChain ch, const int32_t *tok, int q_lo, const int32_t *base, const int32_t *first,
                                                    const int32_t *chb, int32_t *lk_start, int32_t *lk_pos)
{
    __shared__ int tile[256];
    const int B = ch.B, V = ch.V;
    const int q = q_lo + blockIdx.x, bg = blockIdx.y * 256, b = bg + (int)threadIdx.x;
    const int v = b < B ? chain_token(ch, tok, tok, nullptr, q, b) : -1;
    int rank = 0;
    for (int j0 = 0; j0 < min(B, bg + 256); j0 += 256) {
        __syncthreads();
        const int j = j0 + (int)threadIdx.x;
        tile[threadIdx.x] = j < B ? chain_token(ch, tok, tok, nullptr, q, j) : 0;
        __syncthreads();
        const int lim = min(256, b - j0);
        for (int k = 0; k < lim; ++k) rank += tile[k] == v ? 1 : 0;
    }
    if (b >= B) return;
    const int p = base[(size_t)q * (V + 2) + v] + rank, slot = first[v] + p;
    lk_pos[slot] = q * B + b;
    if (p % NVQA_AE_LK_CHUNK == 0) lk_start[chb[v] + p / NVQA_AE_LK_CHUNK] = slot;
}

// The six update rules of misc/optim_updates.lua, one element each; RULE = NVQA_OPT_*.  alpha / beta are b1 / b2, step is Adam's
// bias-corrected rate (formed on the host), m is the rule's one state buffer (Adam: m and v).  RMSPROP keeps k_rmsprop's
// expressions (kernels.h) term for term: nvqa_rmsprop_update and nvqa_optim_update share the buffer and must give the same bits.
struct RuleArgs {
    float lr, b1, b2, eps, step;
};
template <int RULE>
__device__ __forceinline__ void rule_apply(const RuleArgs &r, float &x, float &m, float &v, float g)
{
    if constexpr (RULE == NVQA_OPT_SGD) {           // :4-10
        x += -r.lr * g;
    } else if constexpr (RULE == NVQA_OPT_SGDM) {   // :12-24
        m = r.b1 * m + r.lr * g;
        x -= m;
    } else if constexpr (RULE == NVQA_OPT_SGDMOM) { // :26-40
        const float m0 = m;
        m = r.b1 * m0 - r.lr * g;
        x += -r.b1 * m0;
        x += (1.f + r.b1) * m;
    } else if constexpr (RULE == NVQA_OPT_ADAGRAD) { // :42-57
        m += g * g;
        x += -r.lr * g / (sqrtf(m) + r.eps);
    } else if constexpr (RULE == NVQA_OPT_RMSPROP) { // :60-76
        const float om = 1.0f - r.b1;
        const float mi = r.b1 * m + om * g * g;
        m = mi;
        x += -r.lr * g / (sqrtf(mi) + r.eps);
    } else {                                         // :78-111
        m = r.b1 * m + (1.f - r.b1) * g;
        v = r.b2 * v + (1.f - r.b2) * g * g;
        x -= r.step * (m / (sqrtf(v) + r.eps));
    }
}
template <int RULE> struct RuleState { // how many state buffers the rule reads and writes
    static constexpr int n = RULE == NVQA_OPT_SGD ? 0 : (RULE == NVQA_OPT_ADAM ? 2 : 1);
};

// clamp -> + wd x -> the rule in one pass, with the log line's statistics of x before the update:
// part[2 blk] = sum x^2, part[2 blk + 1] = count(|lr g| >= 0.01 |x|).  Per-segment gradient scales (data-parallel mean,
// -lr_scale) are applied before the clamp as k_rmsprop does; the step-skip words are honoured like there.
// HBM traffic per parameter: 12 B (SGD: read x, g; write x), 20 B (one state buffer), 28 B (Adam).
struct OptimArgs {
    float *x, *m, *v;
    const float *g;
    size_t n, seg0, seg1; // segment ends: [0, seg0) scale gs[0], [seg0, seg1) gs[1], rest gs[2]
    float gs[3];
    RuleArgs r;
    float wd, clamp;
    const unsigned *skip;
    const float *dp_skip;
    float *h_dp, *dp_next;
    double *part;
};
template <int RULE>
__device__ __forceinline__ void optim_one(const OptimArgs &a, size_t i, float &x, float &m, float &v, float g, double &sq, double &cnt)
{
    g *= i < a.seg0 ? a.gs[0] : (i < a.seg1 ? a.gs[1] : a.gs[2]);
    if (a.clamp > 0.f) g = fminf(fmaxf(g, -a.clamp), a.clamp);
    if (a.wd != 0.f) g += a.wd * x;
    sq += (double)x * (double)x;
    cnt += fabsf(g * a.r.lr) >= fabsf(x) * 0.01f ? 1.0 : 0.0;
    rule_apply<RULE>(a.r, x, m, v, g);
}
// the block's two partial sums -> part[2 blk], part[2 blk + 1]
__device__ __forceinline__ void optim_stats_out(double (*sh)[256], double sq, double cnt, double *part)
{
    sh[0][threadIdx.x] = sq;
    sh[1][threadIdx.x] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if ((int)threadIdx.x < o) { sh[0][threadIdx.x] += sh[0][threadIdx.x + o]; sh[1][threadIdx.x] += sh[1][threadIdx.x + o]; }
        __syncthreads();
    }
    if (threadIdx.x == 0) { part[2 * blockIdx.x] = sh[0][0]; part[2 * blockIdx.x + 1] = sh[1][0]; }
}
template <int RULE>
__global__ __launch_bounds__(256) void k_optim(OptimArgs a)
{
    constexpr int NS = RuleState<RULE>::n;
    __shared__ double sh[2][256];
    if (a.dp_next && blockIdx.x == 0 && threadIdx.x == 0) *a.dp_next = 0.f;
    bool skip = a.skip && (a.skip[0] | a.skip[4]) != 0u;
    if (a.dp_skip && a.dp_skip[0] != 0.f) {
        if (a.h_dp && blockIdx.x == 0 && threadIdx.x == 0) __hip_atomic_store(a.h_dp + 1, a.dp_skip[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        skip = true;
    }
    double sq = 0, cnt = 0;
    if (!skip) {
        const size_t n4 = a.n / 4, stride = (size_t)gridDim.x * blockDim.x;
        float4 *x4 = reinterpret_cast<float4 *>(a.x), *m4 = reinterpret_cast<float4 *>(a.m), *v4 = reinterpret_cast<float4 *>(a.v);
        const float4 *g4 = reinterpret_cast<const float4 *>(a.g);
        for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n4; i += stride) {
            float4 xv = x4[i], mv = {}, vv = {};
            if constexpr (NS >= 1) mv = m4[i];
            if constexpr (NS >= 2) vv = v4[i];
            const float4 gv = g4[i];
            optim_one<RULE>(a, 4 * i + 0, xv.x, mv.x, vv.x, gv.x, sq, cnt);
            optim_one<RULE>(a, 4 * i + 1, xv.y, mv.y, vv.y, gv.y, sq, cnt);
            optim_one<RULE>(a, 4 * i + 2, xv.z, mv.z, vv.z, gv.z, sq, cnt);
            optim_one<RULE>(a, 4 * i + 3, xv.w, mv.w, vv.w, gv.w, sq, cnt);
            x4[i] = xv;
            if constexpr (NS >= 1) m4[i] = mv;
            if constexpr (NS >= 2) v4[i] = vv;
        }
        const size_t t = 4 * n4 + (size_t)blockIdx.x * blockDim.x + threadIdx.x; // the < 4 trailing elements
        if (t < a.n) {
            float m = 0.f, v = 0.f;
            if constexpr (NS >= 1) m = a.m[t];
            if constexpr (NS >= 2) v = a.v[t];
            optim_one<RULE>(a, t, a.x[t], m, v, a.g[t], sq, cnt);
            if constexpr (NS >= 1) a.m[t] = m;
            if constexpr (NS >= 2) a.v[t] = v;
        }
    }
    if (a.part) optim_stats_out(sh, sq, cnt, a.part);
}

// the weak-paired AE's projection update (the cnn branch of 004_train_arch2_weakpaired_autoencoder_vgg.lua: g += wd x, then
// clamp (:318-322), then sgd / sgdm / adam of misc/optim_updates.lua with lrs = 1, cnnFinalLearningScales of the final Linear),
// over x = [W_p | b_p], n values; part[2 blk] = sum x^2 of the weight (i < nw: cnn:get(40).weight), part[2 blk + 1] =
// count(|lr g| >= 0.01 |x|) over all n (:302-305), both of x before the update
template <int RULE>
__global__ __launch_bounds__(256) void k_ae_wp_optim(float *x, float *m, float *v, const float *g, size_t n, size_t nw, RuleArgs r,
                                                     float wd, float clamp, double *part)
{
    constexpr int NS = RuleState<RULE>::n;
    __shared__ double sh[2][256];
    double sq = 0, cnt = 0;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float xi = x[i];
        float gi = g[i];
        if (wd != 0.f) gi += wd * xi;
        if (clamp > 0.f) gi = fminf(fmaxf(gi, -clamp), clamp);
        if (i < nw) sq += (double)xi * (double)xi;
        cnt += fabsf(gi * r.lr) >= fabsf(xi) * 0.01f ? 1.0 : 0.0;
        float xo = xi, mi = 0.f, vi = 0.f;
        if constexpr (NS >= 1) mi = m[i];
        if constexpr (NS >= 2) vi = v[i];
        rule_apply<RULE>(r, xo, mi, vi, gi);
        if constexpr (NS >= 1) m[i] = mi;
        if constexpr (NS >= 2) v[i] = vi;
        x[i] = xo;
    }
    if (part) optim_stats_out(sh, sq, cnt, part);
}

// ------------------------------------------------------------------------------------------------------------------
// GEMM configurations (gemm_f32.h).  Projection and time-batched products: 128 x 128 tiles (16x16x4 MFMA, 8 waves) for
// the short-K forms, the 4-wave 32x32x2 form for the long-K weight gradients (the choice nvqa_api.hip measured for the same
// product shapes); recurrent steps: the VQA per-level configurations.
// ------------------------------------------------------------------------------------------------------------------
typedef Cfg<16, 128, 128, 32, 4, 2, 1, 1> AeCfgWide;
typedef Cfg<32, 128, 128, 32, 2, 2, 1, 1> AeCfgLongK;
typedef Cfg<16, 64, 64, 64, 4, 1, 2, 1> AeCfgGates;  // = CfgLstmFwd
typedef Cfg<16, 64, 32, 64, 4, 2, 1, 1> AeCfgStepBwd; // = CfgNarrow
// bf16 operand mode, projection group: both operands bf16 in memory, K-contiguous (gemm_f32.h BF = 2: sizes in pairs of bf16)
typedef Cfg<16, 128, 128, 32, 4, 2, 1, 1, 0, 0, 2, 1> AeCfgImg; // = CfgDx0B

#define AE_LAUNCH(CFG, AM, BM, GATES, EPI, SEG, g, e) NVQA_HIP((launch_gemm<CFG, AM, BM, GATES, EPI, SEG>(c->s, g, e)))
// a product of the AE1 / AE2 chain: in the bf16 operand mode the BF = 1 instance of the same configuration (f32 in memory, both
// operands rounded to bf16 at the fragment read, one bf16 MFMA per four f32 ones, f32 accumulate); else the f32 kernel as ever
#define AE_LAUNCH_P(CFG, AM, BM, GATES, EPI, SEG, g, e)                          \
    do {                                                                         \
        if (c->ae->bf16) AE_LAUNCH(WithBF<CFG>::type, AM, BM, GATES, EPI, SEG, g, e); \
        else AE_LAUNCH(CFG, AM, BM, GATES, EPI, SEG, g, e);                      \
    } while (0)

// dlogits (bf16 operand mode): X = the logits, summed as (softmax - onehot) / n through the rows' log-sum-exp and target
static int colsum(nvqa_ctx *c, const float *X, int M, int N, int ld, float *out, float *out2, bool dlogits = false)
{
    AeState &a = *c->ae;
    int S = std::min(64, std::max(1, M / 256));
    const int rps = (M + S - 1) / S;
    S = (M + rps - 1) / rps;
    if ((size_t)S * N > a.colpart_floats) { set_error("ae: column-sum scratch too small"); return -1; }
    if (dlogits)
        hipLaunchKernelGGL(k_ae_colsum_dlogits_part, dim3((N + 255) / 256, S), dim3(256), 0, c->s, X, (const float *)a.rowlse,
                           (const int32_t *)a.rowtgt, a.inv_n, a.wcur, M, N, ld, rps, a.colpart);
    else
        hipLaunchKernelGGL(k_ae_colsum_part, dim3((N + 255) / 256, S), dim3(256), 0, c->s, X, M, N, ld, rps, a.colpart);
    hipLaunchKernelGGL(k_ae_colsum_final, dim3((N + 255) / 256), dim3(256), 0, c->s, a.colpart, S, N, out, out2);
    NVQA_HIP(hipGetLastError());
    return 0;
}

// out [M x N] = A^T B summed over K rows: A stored [K][M] (lda), B stored [K][N] (ldb); split-K into slabs, fixed-order sum
// bf16 operand mode: the K-major gfx950 kernel of wgrad_bf16.h instead, which rounds the f32 rows to bf16 on their way into LDS
// or, given A16 / B16 (both), stages from bf16 images with the same leading dimensions
static int wgrad(nvqa_ctx *c, const float *A, int lda, const float *Bm, int ldb, int M, int N, int K, float *out,
                 const unsigned short *A16 = nullptr, const unsigned short *B16 = nullptr)
{
    AeState &a = *c->ae;
    if (K <= 0) {
        NVQA_HIP(hipMemsetAsync(out, 0, (size_t)M * N * 4, c->s));
        return 0;
    }
    const int tiles = ((M + 127) / 128) * ((N + 127) / 128);
    int Z = std::max(1, std::min(16, 512 / std::max(tiles, 1)));
    while (Z > 1 && (size_t)Z * M * N > a.slab_floats) --Z;
    const int kq = a.bf16 ? NVQA_WB_BK : 32;
    const int kslice = ((K + Z - 1) / Z + kq - 1) / kq * kq;
    Z = (K + kslice - 1) / kslice;
    if (a.bf16) {
        if (!A16 || !B16) A16 = B16 = nullptr; // both images or neither
        NVQA_HIP(wgrad_bf16_launch(c->s, WgradBf16Args{A, Bm, A16, B16, Z > 1 ? a.slabs : out, Z > 1 ? (size_t)M * N : 0, lda, ldb, N, M, N, K, kslice}));
    } else {
        GemmArgs g = ae_args(A, lda, Bm, ldb, M, N, K, kslice);
        const EpiStore e{Z > 1 ? a.slabs : out, N, (size_t)M * N};
        AE_LAUNCH(AeCfgLongK, A_MC, B_NC, false, EpiStore, 0, g, e);
    }
    if (Z > 1) {
        hipLaunchKernelGGL(k_ae_slab_sum, dim3(1024), dim3(256), 0, c->s, a.slabs, Z, (size_t)M * N, out);
        NVQA_HIP(hipGetLastError());
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------------------------
// lifetime
// ------------------------------------------------------------------------------------------------------------------
int ae_create(nvqa_ctx *c)
{
    const nvqa_dims &d = c->d;
    NVQA_HIP(hipStreamCreateWithFlags(&c->s, hipStreamNonBlocking));
    c->ae = new AeState();
    AeState &a = *c->ae;
    const size_t B = d.B, D = d.T, E = d.E, R = d.R, L = d.L, V = d.V;
    a.ae2 = d.arch == NVQA_ARCH_AE2 || d.arch == NVQA_ARCH_AE2_WP;
    a.wp = d.arch == NVQA_ARCH_AE2_WP;
    a.bridge = d.arch == NVQA_ARCH_AE1_WP;
    a.feats = a.wp || a.bridge;
    a.flags = (a.ae2 ? AE_CHAIN_AE2 : 0) | (a.bridge ? AE_CHAIN_BRIDGE : 0) | (a.feats ? AE_CHAIN_ENC : 0);
    a.D = (int)D;
    a.QM = (int)(2 * D + (a.ae2 ? 3 : 1));
    a.dstr = (int)D + (a.ae2 ? 1 : 0);
    a.ldl = (int)((V + 1 + 3) / 4 * 4);
    const size_t QM = a.QM, total4 = (c->lo.total + 3) / 4 * 4; // (padding: nvqa_rmsprop_update runs over whole float4s)
    if (a.bridge) {
        // device order [encoder | decoder but b_proj | multimodal | b_proj]: b_proj has V + 1 entries, and the products read W_q and
        // W_v in 16-byte pieces (nvqa_api.hip converts at the ABI); the frozen lookup table sits behind the (padded) vector
        const size_t nb = V + 1;
        c->lo.w_q -= nb; c->lo.b_q -= nb; c->lo.w_v -= nb; c->lo.b_v -= nb;
        c->lo.b_proj = c->lo.total - nb;
        c->lo.w_lk = total4;
    }
    NVQA_TRY(ae_alloc(nullptr, (void **)&c->P, (total4 + (a.bridge ? (V + 1) * E : 0)) * 4)); // (these three are nvqa_destroy's)
    NVQA_TRY(ae_alloc(nullptr, (void **)&c->G, total4 * 4));
    NVQA_TRY(ae_alloc(nullptr, (void **)&c->M2, total4 * 4));
    AE_ALLOC(a.tok, B * D);
    AE_ALLOC(a.nrows, 1);
    {
        const int32_t nb = d.B;
        NVQA_HIP(hipMemcpy(a.nrows, &nb, 4, hipMemcpyHostToDevice));
    }
    AE_ALLOC(a.cur, B);
    AE_ALLOC(a.samples, B * D);
    if (!a.feats) { // the frozen lookup of the weak-paired archs takes no gradient
        AE_ALLOC(a.lk_tok, QM * B);
        AE_ALLOC(a.lk_tc, QM * B + 1);
        AE_ALLOC(a.lk_start, QM * B + 1);
        AE_ALLOC(a.lk_pos, QM * B);
        AE_ALLOC(a.lk_part, QM * B * E);
        AE_PINNED(a.h_lk, 4 * QM * B + 4);
    }
    AE_PINNED(a.h_tok, B * D);
    AE_PINNED(a.h_loss, 4);
    if (a.ae2 && !a.wp) {
        AE_ALLOC(a.img, B * E);
        AE_PINNED(a.h_img, B * E);
    }
    if (a.feats) {
        const size_t I = d.I;
        AE_ALLOC(a.etok, B * D);
        AE_PINNED(a.h_etok, B * D);
        AE_ALLOC(a.feat, B * I);
        AE_PINNED(a.h_feat, B * I);
        NVQA_HIP(hipEventCreateWithFlags(&a.staged, hipEventDisableTiming));
    }
    if (a.bridge) {
        const size_t I = d.I, N = 2 * R;
        int cus = 0;
        NVQA_HIP(hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, c->device));
        a.plan = ae1wp_bridge_plan((int)B, (int)N, (int)N, (int)I, cus > 0 ? cus : 256);
        AE_ALLOC(a.jbuf, B * N);
        AE_PINNED(a.h_j, B * N);
        AE_ALLOC(a.qd, B * N);
        AE_ALLOC(a.vd, B * I);
        AE_ALLOC(a.qc, B * N);
        AE_ALLOC(a.ic, B * N);
        AE_ALLOC(a.dqp, B * N);
        AE_ALLOC(a.dvp, B * N);
        AE_ALLOC(a.dh0, B * R);
        AE_ALLOC(a.dfeat, B * I);
        AE_ALLOC(a.br_slabs, (size_t)(a.plan.zq + a.plan.zv) * B * N);
    }
    if (a.wp) {
        const size_t I = d.I, NP = E * I + E;
        AE_ALLOC(a.wp_x, NP);
        AE_ALLOC(a.wp_g, NP);
        AE_ALLOC(a.wp_m, NP);
        AE_ALLOC(a.wp_v, NP);
        AE_ALLOC(a.wp_part, 2 * 1024);
    }
    AE_ALLOC(a.X0, QM * B * E);
    for (size_t l = 0; l < L; ++l) {
        AE_ALLOC(a.Gt[l], QM * B * 4 * R);
        AE_ALLOC(a.Hs[l], (QM + 1 + (a.bridge ? 1 : 0)) * B * R);
        AE_ALLOC(a.Cs[l], (QM + 1 + (a.bridge ? 1 : 0)) * B * R);
        if (l > 0) AE_ALLOC(a.U[l], QM * B * R);
    }
    AE_ALLOC(a.dX, QM * B * std::max(E, R));
    AE_ALLOC(a.dHx, QM * B * R);
    AE_ALLOC(a.dc, B * R);
    AE_ALLOC(a.Htd, (D + 1) * B * R);
    AE_ALLOC(a.logits, (D + 1) * B * (size_t)a.ldl);
    AE_ALLOC(a.rowloss, (D + 1) * B);
    AE_ALLOC(a.loss, 4);
    AE_ALLOC(a.dpw, 4);
    {
        const float one[2] = {1.f, 1.f};
        NVQA_HIP(hipMemcpy(a.dpw + 2, one, 8, hipMemcpyHostToDevice));
    }
    a.wcur = a.dpw + 3;
    a.slab_floats = (size_t)8 * 4 * R * std::max(E, R);
    if (a.bridge) a.slab_floats = std::max(a.slab_floats, (size_t)2 * R * std::max<size_t>(2 * R, d.I)); // dW_q, dW_v: at least one slab
    AE_ALLOC(a.slabs, a.slab_floats);
    a.colpart_floats = (size_t)64 * std::max<size_t>(4 * R, V + 1);
    AE_ALLOC(a.colpart, a.colpart_floats);
    return 0;
}

void ae_destroy(nvqa_ctx *c)
{
    if (!c->ae) return;
    AeState &a = *c->ae;
    for (void *p : a.dev) (void)hipFree(p);
    for (void *p : a.pinned) (void)hipHostFree(p);
    if (a.corpus) (void)hipFree(a.corpus);
    if (a.staged) (void)hipEventDestroy(a.staged);
    if (a.step_ev) (void)hipEventDestroy(a.step_ev);
    delete c->ae;
    c->ae = nullptr;
}

// ------------------------------------------------------------------------------------------------------------------
// forward / backward
// ------------------------------------------------------------------------------------------------------------------
// weights of chain step q: the encoder's below te, the decoder's from te on
static inline size_t w_i2h_of(const nvqa_ctx *c, int l, bool dec) { return dec ? c->lo.d_w_i2h[l] : c->lo.w_i2h[l]; }
static inline size_t w_h2h_of(const nvqa_ctx *c, int l, bool dec) { return dec ? c->lo.d_w_h2h[l] : c->lo.w_h2h[l]; }

// time-batched input projection of layer l for chain steps [q0, q1) (all of one phase) + both biases
static int ae_i2h(nvqa_ctx *c, int l, int q0, int q1, bool dec)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R, in = l == 0 ? c->d.E : R;
    if (q1 <= q0) return 0;
    const float *X = (l == 0 ? a.X0 : a.U[l]) + (size_t)q0 * B * in;
    const int M = (q1 - q0) * B;
    ProfScope ps(c, PF_AE_I2H, 2.0 * M * 4 * R * in);
    GemmArgs g = ae_args(X, in, c->P + w_i2h_of(c, l, dec), in, M, 4 * R, in);
    const EpiBias2 e{a.Gt[l] + (size_t)q0 * B * 4 * R, 4 * R, c->P + (dec ? c->lo.d_b_i2h[l] : c->lo.b_i2h[l]),
                     c->P + (dec ? c->lo.d_b_h2h[l] : c->lo.b_h2h[l])};
    AE_LAUNCH_P(AeCfgWide, A_KC, B_KC, false, EpiBias2, 0, g, e);
    return 0;
}

// recurrent step q of layer l: gates = (projection in Gt) + h_{q-1} W_h2h^T, fused cell (epilogues.h EpiLstmFwd).
// h_from / c_from (beam search): the state the step reads, in place of slot q
static int ae_fwd_step(nvqa_ctx *c, int l, int q, const Drop &dr, const float *h_from = nullptr, const float *c_from = nullptr)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R;
    const bool dec = q >= a.te;
    const int sl = q + (a.bridge && dec ? 1 : 0); // state slot step q reads
    const bool h_in = q > 0 || (a.bridge && dec); // h_{-1} = 0 but for a decoder that starts from the bridge
    ProfScope ps(c, PF_AE_LSTM_FWD, h_in ? 2.0 * B * 4 * R * R : 0.0);
    EpiLstmFwd e = {};
    e.gx = a.Gt[l] + (size_t)q * B * 4 * R;
    e.c_prev = c_from ? c_from : a.Cs[l] + (size_t)sl * B * R;
    e.c = a.Cs[l] + (size_t)(sl + 1) * B * R;
    e.h = a.Hs[l] + (size_t)(sl + 1) * B * R;
    e.nrows = a.nrows;
    e.R = R; e.B = B; e.T = a.QM; e.t = q; e.lnext_m1 = l;
    e.dr = dr;
    const float *hprev = h_from ? h_from : a.Hs[l] + (size_t)sl * B * R;
    GemmArgs g = ae_args(hprev, R, c->P + w_h2h_of(c, l, dec), R, B, R, 0);
    g.R = R;
    g.A2 = hprev; g.lda2 = R; g.B2 = c->P + w_h2h_of(c, l, dec); g.ldb2 = R; g.K2 = h_in ? R : 0;
    AE_LAUNCH_P(AeCfgGates, A_KC, B_KC, true, EpiLstmFwd, 1, g, e);
    return 0;
}

// input of layer l >= 1 for chain steps [q0, q1): Dropout(h of layer l-1) (LSTM_encoder.lua / LSTM_decoder.lua drop_L)
static int ae_layer_input(nvqa_ctx *c, int l, int q0, int q1, const Drop &dr)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R;
    const size_t n = (size_t)(q1 - q0) * B * R;
    hipLaunchKernelGGL(k_ae_drop<false>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->s,
                       a.Hs[l - 1] + (size_t)(q0 + 1) * B * R, a.U[l] + (size_t)q0 * B * R, n, R, B, a.dstr, c->d.L, l, a.te,
                       q0 * B, 0, dr, (unsigned short *)nullptr);
    NVQA_HIP(hipGetLastError());
    return 0;
}

// logits of decoder steps [s0, s1): Dropout(top h) -> Linear(R, V+1)
static int ae_project(nvqa_ctx *c, int s0, int s1, const Drop &dr)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R, L = c->d.L, Vp1 = c->d.V + 1;
    const size_t n = (size_t)(s1 - s0) * B * R;
    const float *htop = a.Hs[L - 1] + (size_t)(a.te + 1 + (a.bridge ? 1 : 0) + s0) * B * R;
    const dim3 dgrid((unsigned)std::min<size_t>((n + 255) / 256, 4096));
    if (a.p16)
        hipLaunchKernelGGL(k_ae_drop<true>, dgrid, dim3(256), 0, c->s, htop, a.Htd + (size_t)s0 * B * R, n, R, B, a.dstr, L, 0, 0,
                           s0 * B, 1, dr, a.Htd16 + (size_t)s0 * B * R);
    else
        hipLaunchKernelGGL(k_ae_drop<false>, dgrid, dim3(256), 0, c->s, htop, a.Htd + (size_t)s0 * B * R, n, R, B, a.dstr, L, 0, 0,
                           s0 * B, 1, dr, (unsigned short *)nullptr);
    NVQA_HIP(hipGetLastError());
    const int M = (s1 - s0) * B;
    ProfScope ps(c, PF_AE_PROJ_FWD, 2.0 * M * (double)Vp1 * R);
    if (a.p16) { // both operands from their bf16 images (sizes in pairs of bf16); the f32 logits as ever
        GemmArgs g = ae_args(reinterpret_cast<const float *>(a.Htd16 + (size_t)s0 * B * R), R / 2, reinterpret_cast<const float *>(a.Wp16),
                             R / 2, M, Vp1, R / 2);
        const EpiAeBias e{a.logits + (size_t)s0 * B * a.ldl, a.ldl, c->P + c->lo.b_proj};
        AE_LAUNCH(AeCfgImg, A_KC, B_KC, false, EpiAeBias, 0, g, e);
        return 0;
    }
    GemmArgs g = ae_args(a.Htd + (size_t)s0 * B * R, R, c->P + c->lo.w_proj, R, M, Vp1, R);
    const EpiAeBias e{a.logits + (size_t)s0 * B * a.ldl, a.ldl, c->P + c->lo.b_proj};
    AE_LAUNCH_P(AeCfgWide, A_KC, B_KC, false, EpiAeBias, 0, g, e);
    return 0;
}

static inline AeChain ae_chain(const nvqa_ctx *c) { return {c->d.B, c->ae->D, c->d.V, c->ae->te, c->ae->tmax + 1, c->ae->flags}; }

// layer-0 inputs of chain steps [q0, q1): one launch.  The weak-paired archs read the encoder's tokens from etok and run the
// frozen lookup evaluate()d (AE1_WP: no mask, AutoEncoder_vqa_arch.lua:133-134); AE2_WP's chain row 0 is ae_wp_project's
static int ae_embed(nvqa_ctx *c, int q0, int q1, const int32_t *direct, const Drop &dr)
{
    AeState &a = *c->ae;
    const nvqa_dims &d = c->d;
    if (a.wp) q0 = std::max(q0, 1);
    if (q1 <= q0) return 0;
    ProfScope ps(c, PF_AE_EMB, 0, (double)(q1 - q0) * d.B * d.E * 8);
    const dim3 grid((unsigned)((q1 - q0) * d.B)), nt(std::min(256, (d.E + 63) / 64 * 64));
    const int32_t *enc = a.feats ? a.etok : a.tok;
    if (a.ae2)
        hipLaunchKernelGGL(k_ae2_assemble, grid, nt, 0, c->s, ae_chain(c), enc, (const int32_t *)a.tok, direct,
                           (const float *)(a.img_live ? a.img : nullptr), d.E, q0, c->P + c->lo.w_lk, a.X0);
    else
        hipLaunchKernelGGL(k_ae_embed, grid, nt, 0, c->s, ae_chain(c), enc, (const int32_t *)a.tok, direct, d.E, q0, c->P + c->lo.w_lk,
                           a.bridge ? ae_drop(nullptr, false) : dr, a.X0);
    NVQA_HIP(hipGetLastError());
    return 0;
}

// AE2_WP: chain step 0 of X0 = f^ W_p^T + b_p (build_cnn's final Linear, misc/net_utils.lua:37-41), one GEMM M = B, N = E, K = I
static int ae_wp_project(nvqa_ctx *c)
{
    AeState &a = *c->ae;
    const int B = c->d.B, E = c->d.E, I = c->d.I;
    ProfScope ps(c, PF_AE_WP_PROJ_FWD, 2.0 * B * E * (double)I);
    GemmArgs g = ae_args(a.feat, I, a.wp_x, I, B, E, I);
    const EpiAeBias e{a.X0, E, a.wp_x + (size_t)E * I};
    AE_LAUNCH(AeCfgWide, A_KC, B_KC, false, EpiAeBias, 0, g, e);
    return 0;
}

// AE1_WP: the bridge (ae_bridge.h) from the encoder's final slot te (or the caller's j: skip) into the decoder's slot te + 1
static int ae_bridge_forward(nvqa_ctx *c, const Drop &dr)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R, I = c->d.I, N = 2 * R;
    const BridgePlan &pl = a.plan;
    ProfScope ps(c, PF_AE1WP_BRIDGE_FWD, 2.0 * B * N * (double)(N + I), 4.0 * N * (double)(N + I));
    const size_t sl = (size_t)a.te * B * R;
    hipLaunchKernelGGL(k_ae1wp_bridge_prep, dim3((unsigned)std::min<size_t>(((size_t)B * (N + I) + 255) / 256, 2048)), dim3(256), 0, c->s,
                       a.skip ? (const float *)nullptr : a.Cs[0] + sl, a.skip ? (const float *)nullptr : a.Hs[0] + sl, a.jbuf,
                       (const float *)a.feat, B, R, I, dr, a.qd, a.vd);
    NVQA_HIP(hipGetLastError());
    float *sq = a.br_slabs, *sv = a.br_slabs + (size_t)pl.zq * B * N;
    const float *Wq = c->P + c->lo.w_q, *Wv = c->P + c->lo.w_v;
    if (pl.skinny) {
        BridgeGemvArgs g = {};
        g.x[0] = a.qd; g.x[1] = a.vd; g.w[0] = Wq; g.w[1] = Wv; g.slab[0] = sq; g.slab[1] = sv;
        g.K[0] = N; g.K[1] = I; g.Z[0] = pl.zq; g.Z[1] = pl.zv; g.B = B; g.N = N; g.ks = pl.ks;
        hipLaunchKernelGGL(k_ae1wp_bridge_gemv, dim3((unsigned)pl.workgroups), dim3(256), 0, c->s, g);
        NVQA_HIP(hipGetLastError());
    } else {
        GemmArgs gq = ae_args(a.qd, N, Wq, N, B, N, N, pl.ks), gv = ae_args(a.vd, I, Wv, I, B, N, I, pl.ks);
        const EpiStore eq{sq, N, (size_t)B * N}, ev{sv, N, (size_t)B * N};
        AE_LAUNCH(AeCfgWide, A_KC, B_KC, false, EpiStore, 0, gq, eq);
        AE_LAUNCH(AeCfgWide, A_KC, B_KC, false, EpiStore, 0, gv, ev);
    }
    hipLaunchKernelGGL(k_ae1wp_bridge_fwd, dim3((unsigned)(((size_t)B * N + 255) / 256)), dim3(256), 0, c->s, (const float *)sq, pl.zq,
                       (const float *)sv, pl.zv, B, R, c->P + c->lo.b_q, c->P + c->lo.b_v, (const float *)a.jbuf, dr, a.qc, a.ic,
                       a.Cs[0] + sl + (size_t)B * R, a.Hs[0] + sl + (size_t)B * R);
    NVQA_HIP(hipGetLastError());
    return 0;
}

// AE1_WP, behind the backward of decoder step 0 (chain step te): a.dc = dc0, Gt[te] = that step's dG.  dh0 = dG W_h2h (the
// decoder's), the bridge's backward, its weight gradients, and -- if the encoder ran -- dc_T into a.dc and dh_T into the
// encoder's last row block of dHx.  want_df: df^ into a.dfeat.
static int ae_bridge_backward(nvqa_ctx *c, const Drop &dr, bool want_df)
{
    AeState &a = *c->ae;
    const int B = c->d.B, R = c->d.R, I = c->d.I, N = 2 * R, TE = a.te;
    ProfScope ps(c, PF_AE1WP_BRIDGE_BWD, 2.0 * B * 4 * R * R + 2.0 * B * N * (double)(N + I) * (want_df ? 2 : 1) + (a.skip ? 0.0 : 2.0 * B * N * N));
    {
        GemmArgs g = ae_args(a.Gt[0] + (size_t)TE * B * 4 * R, 4 * R, c->P + c->lo.d_w_h2h[0], R, B, R, 4 * R);
        const EpiStore e{a.dh0, R, 0};
        AE_LAUNCH(AeCfgStepBwd, A_KC, B_NC, false, EpiStore, 0, g, e);
    }
    hipLaunchKernelGGL(k_ae1wp_bridge_bwd, dim3((unsigned)(((size_t)B * N + 255) / 256)), dim3(256), 0, c->s, (const float *)a.dc,
                       (const float *)a.dh0, (const float *)a.qc, (const float *)a.ic, B, R, dr, a.dqp, a.dvp);
    NVQA_HIP(hipGetLastError());
    NVQA_TRY(wgrad(c, a.dqp, N, a.qd, N, N, N, B, c->G + c->lo.w_q));
    NVQA_TRY(colsum(c, a.dqp, B, N, N, c->G + c->lo.b_q, nullptr));
    NVQA_TRY(wgrad(c, a.dvp, N, a.vd, I, N, I, B, c->G + c->lo.w_v));
    NVQA_TRY(colsum(c, a.dvp, B, N, N, c->G + c->lo.b_v, nullptr));
    if (!a.skip) {
        GemmArgs g = ae_args(a.dqp, N, c->P + c->lo.w_q, N, B, N, N);
        const EpiAe1wpDj e{a.dc, a.dHx + (size_t)(TE - 1) * B * R, a.dh0, R, dr};
        AE_LAUNCH(AeCfgStepBwd, A_KC, B_NC, false, EpiAe1wpDj, 0, g, e);
    }
    if (want_df) {
        GemmArgs g = ae_args(a.dvp, N, c->P + c->lo.w_v, I, B, I, N);
        const EpiAe1wpDf e{a.dfeat, I, dr};
        AE_LAUNCH(AeCfgWide, A_KC, B_NC, false, EpiAe1wpDf, 0, g, e);
    }
    return 0;
}

// bf16 operand mode: this call's bf16 images of W_proj (the weights do not move before the next step)
static int ae_wproj_images(nvqa_ctx *c)
{
    AeState &a = *c->ae;
    if (!a.p16) return 0;
    ProfScope ps(c, PF_AE_WPROJ_IMG, 0, (c->d.V + 1.0) * c->d.R * 8);
    hipLaunchKernelGGL(k_ae_wproj_images, dim3((a.ld16 + 63) / 64, (c->d.R + 63) / 64), dim3(256), 0, c->s, c->P + c->lo.w_proj,
                       c->d.V + 1, c->d.R, a.ld16, a.Wp16, a.WpT16);
    NVQA_HIP(hipGetLastError());
    return 0;
}

// the encoder alone, chain steps [0, te) of every layer: the launches of ae_forward on the encoder's own row counts
static int ae_run_encoder(nvqa_ctx *c, const Drop &dr)
{
    const int te = c->ae->te;
    NVQA_TRY(ae_embed(c, 0, te, nullptr, dr));
    for (int l = 0; l < c->d.L; ++l) {
        if (l > 0) NVQA_TRY(ae_layer_input(c, l, 0, te, dr));
        NVQA_TRY(ae_i2h(c, l, 0, te, false));
        for (int q = 0; q < te; ++q) NVQA_TRY(ae_fwd_step(c, l, q, dr));
    }
    return 0;
}

// decoder step s alone, fed START (s = 0) or direct[b], down to its logits.  beam: the step reads bm_h / bm_c, not its state slot
static int ae_decode_step(nvqa_ctx *c, int s, const int32_t *direct, bool beam)
{
    AeState &a = *c->ae;
    const Drop dr = ae_drop(nullptr, false);
    const int q = a.te + s;
    NVQA_TRY(ae_embed(c, q, q + 1, s == 0 ? nullptr : direct, dr));
    for (int l = 0; l < c->d.L; ++l) {
        if (l > 0) NVQA_TRY(ae_layer_input(c, l, q, q + 1, dr));
        NVQA_TRY(ae_i2h(c, l, q, q + 1, true));
        NVQA_TRY(ae_fwd_step(c, l, q, dr, beam ? a.bm_h[l] : nullptr, beam ? a.bm_c[l] : nullptr));
    }
    return ae_project(c, s, s + 1, dr);
}

// teacher-forced forward of the whole chain (training and evaluate mode) + the criterion; grad: d(logits) in place
static int ae_forward(nvqa_ctx *c, const Drop &dr, int nvalid, bool grad)
{
    AeState &a = *c->ae;
    const nvqa_dims &d = c->d;
    const int B = d.B, L = d.L, Q = a.te + a.tmax + 1, Vp1 = d.V + 1, ncount = a.ncount;
    if (a.wp) NVQA_TRY(ae_wp_project(c));
    NVQA_TRY(ae_wproj_images(c)); // (greedy decoding reuses them)
    NVQA_TRY(ae_embed(c, 0, Q, nullptr, dr));
    for (int l = 0; l < L; ++l) {
        if (l > 0) NVQA_TRY(ae_layer_input(c, l, 0, Q, dr));
        NVQA_TRY(ae_i2h(c, l, 0, a.te, false));
        NVQA_TRY(ae_i2h(c, l, a.te, Q, true));
        for (int q = 0; q < Q; ++q) {
            if (a.bridge && q == a.te) NVQA_TRY(ae_bridge_forward(c, dr));
            NVQA_TRY(ae_fwd_step(c, l, q, dr));
        }
    }
    NVQA_TRY(ae_project(c, 0, a.tmax + 1, dr));
    const int rows = (a.tmax + 1) * B;
    a.inv_n = 1.0f / (float)ncount;
    const bool dp = grad && c->comm; // a data-parallel step: rank weight from the exchange, loss partial into the closing one
    a.wcur = dp ? a.dpw + 2 : a.dpw + 3;
    a.loss_global = dp;
    if (a.dp_wait) { // the count's all-reduce had the whole forward pass to finish
        NVQA_HIP(hipStreamWaitEvent(c->s, c->evComm, 0));
        a.dp_wait = false;
    }
    {
        ProfScope ps(c, PF_AE_SOFTMAX, 0, (double)rows * a.ldl * 4 * (grad ? (a.p16 ? 2.5 : 3) : 1));
        if (a.p16 && grad)
            hipLaunchKernelGGL(k_ae_softmax<true>, dim3(rows), dim3(256), 0, c->s, a.logits, a.ldl, Vp1, a.tok, B, a.D, nvalid,
                               1.0f / (float)ncount, a.wcur, 1, a.rowloss, a.G16, a.ld16, a.rowlse, a.rowtgt);
        else
            hipLaunchKernelGGL(k_ae_softmax<false>, dim3(rows), dim3(256), 0, c->s, a.logits, a.ldl, Vp1, a.tok, B, a.D, nvalid,
                               1.0f / (float)ncount, a.wcur, grad ? 1 : 0, a.rowloss, (unsigned short *)nullptr, 0, (float *)nullptr,
                               (int32_t *)nullptr);
        hipLaunchKernelGGL(k_ae_loss, dim3(1), dim3(256), 0, c->s, a.rowloss, rows, 1.0f / (float)ncount, a.wcur,
                           dp ? c->dp_status + 2 : a.loss);
        NVQA_HIP(hipGetLastError());
    }
    if (!dp) NVQA_HIP(hipMemcpyAsync(a.h_loss, a.loss, 4, hipMemcpyDeviceToHost, c->s));
    return 0;
}

static int ae_backward(nvqa_ctx *c, const Drop &dr, bool want_df = false)
{
    AeState &a = *c->ae;
    const nvqa_dims &d = c->d;
    const int B = d.B, R = d.R, E = d.E, L = d.L, Vp1 = d.V + 1, T = a.tmax, TE = a.te, Q = TE + T + 1;
    const int rows = (T + 1) * B;
    // projection: dH_top (through drop_final) into the decoder rows of dHx, dW_proj, db_proj
    if (TE > 0) NVQA_HIP(hipMemsetAsync(a.dHx, 0, (size_t)TE * B * R * 4, c->s)); // the encoder's rows: no loss reaches them directly
    if (a.p16) {
        // from the bf16 images: dH_top = G16 WpT16^T (K = V + 1 contiguous in both, zero padding up to ld16), dW_proj = G16^T Htd16
        // (K = rows, both K-major); db_proj sums the f32 values (k_ae_colsum_dlogits_part) in colsum's order
        ProfScope ps(c, PF_AE_PROJ_BWD, 4.0 * rows * (double)Vp1 * R);
        GemmArgs g = ae_args(reinterpret_cast<const float *>(a.G16), a.ld16 / 2, reinterpret_cast<const float *>(a.WpT16), a.ld16 / 2,
                             rows, R, a.ld16 / 2);
        const EpiAeTop e{a.dHx + (size_t)TE * B * R, R, B, a.dstr, dr};
        AE_LAUNCH(AeCfgImg, A_KC, B_KC, false, EpiAeTop, 0, g, e);
        NVQA_TRY(wgrad(c, a.logits, a.ld16, a.Htd, R, Vp1, R, rows, c->G + c->lo.w_proj, a.G16, a.Htd16));
        NVQA_TRY(colsum(c, a.logits, rows, Vp1, a.ldl, c->G + c->lo.b_proj, nullptr, true));
    } else {
        ProfScope ps(c, PF_AE_PROJ_BWD, 4.0 * rows * (double)Vp1 * R);
        GemmArgs g = ae_args(a.logits, a.ldl, c->P + c->lo.w_proj, R, rows, R, Vp1);
        const EpiAeTop e{a.dHx + (size_t)TE * B * R, R, B, a.dstr, dr};
        AE_LAUNCH_P(AeCfgLongK, A_KC, B_NC, false, EpiAeTop, 0, g, e);
        NVQA_TRY(wgrad(c, a.logits, a.ldl, a.Htd, R, Vp1, R, rows, c->G + c->lo.w_proj));
        NVQA_TRY(colsum(c, a.logits, rows, Vp1, a.ldl, c->G + c->lo.b_proj, nullptr));
    }
    // data parallel (no-ops without a communicator): W_proj | b_proj is final first and is the largest bucket but for the lookup
    // table; it travels under the whole BPTT chain.  The LSTM slices follow layer by layer, the lookup table last (ae_step_impl joins).
    NVQA_TRY(ae_comm_reduce(c, c->lo.w_proj, c->lo.b_proj + (size_t)Vp1 - c->lo.w_proj, 1));
    for (int l = L - 1; l >= 0; --l) {
        const int in = l == 0 ? E : R;
        NVQA_HIP(hipMemsetAsync(a.dc, 0, (size_t)B * R * 4, c->s));
        for (int q = Q - 1; q >= 0; --q) {
            // dh_q = dG_{q+1} W_h2h (of the phase of step q+1) + dHx_q; cell backward (epilogues.h EpiLstmBwd)
            // (AE1_WP: the encoder's last step gets its dh_T from the bridge through dHx, not from a recurrent product)
            const bool last = q == Q - 1 || (a.bridge && q == TE - 1), dec_next = q + 1 >= TE;
            const int sl = q + (a.bridge && q >= TE ? 1 : 0);
            {
            ProfScope ps(c, PF_AE_LSTM_BWD, last ? 0.0 : 2.0 * B * 4 * R * R);
            EpiLstmBwd e = {};
            e.gates = a.Gt[l] + (size_t)q * B * 4 * R;
            e.c_prev = a.Cs[l] + (size_t)sl * B * R;
            e.c = a.Cs[l] + (size_t)(sl + 1) * B * R;
            e.dc = a.dc;
            e.dh_ext = a.dHx + (size_t)q * B * R;
            e.nrows = a.nrows;
            e.R = R; e.B = B; e.T = a.QM; e.s = q; e.lm1 = 0; e.dr = dr; e.has_upper = 0;
            GemmArgs g = ae_args(last ? a.Gt[l] : a.Gt[l] + (size_t)(q + 1) * B * 4 * R, 4 * R, c->P + w_h2h_of(c, l, dec_next), R,
                                 B, R, last ? 0 : 4 * R);
            AE_LAUNCH_P(AeCfgStepBwd, A_KC, B_NC, false, EpiLstmBwd, 0, g, e);
            }
            if (a.bridge && q == TE) NVQA_TRY(ae_bridge_backward(c, dr, want_df));
        }
        if (!a.bridge) { // d(input) of both phases (AE2_WP, layer 0: chain step 0 only, dx0 -- the frozen lookup takes no gradient;
                         // AE1_WP: frozen lookup and no image row, so nobody reads it)
            const bool cut = a.wp && l == 0;
            ProfScope ps(c, PF_AE_DGRAD, 2.0 * (cut ? 1 : Q) * B * 4.0 * R * in);
            for (int ph = 0; ph < 2; ++ph) {
                const int q0 = ph ? TE : 0, q1 = cut ? (ph ? q0 : 1) : (ph ? Q : TE);
                if (q1 <= q0) continue;
                GemmArgs g = ae_args(a.Gt[l] + (size_t)q0 * B * 4 * R, 4 * R, c->P + w_i2h_of(c, l, ph == 1), in, (q1 - q0) * B, in, 4 * R);
                const EpiStore e{a.dX + (size_t)q0 * B * in, in, 0};
                AE_LAUNCH_P(AeCfgWide, A_KC, B_NC, false, EpiStore, 0, g, e);
            }
        }
        {   // weight and bias gradients of both phases
            ProfScope ps(c, PF_AE_WGRAD, 4.0 * Q * B * 4.0 * R * (in + R));
            for (int ph = 0; ph < 2; ++ph) {
                const int q0 = ph ? TE : 0, q1 = ph ? Q : TE, K = (q1 - q0) * B;
                if (a.bridge && K == 0) { // the encoder was skipped: its gradient segment is exactly zero
                    NVQA_HIP(hipMemsetAsync(c->G, 0, c->lo.seg[0] * 4, c->s));
                    continue;
                }
                const float *dG = a.Gt[l] + (size_t)q0 * B * 4 * R;
                const float *X = (l == 0 ? a.X0 : a.U[l]) + (size_t)q0 * B * in;
                NVQA_TRY(wgrad(c, dG, 4 * R, X, in, 4 * R, in, K, c->G + w_i2h_of(c, l, ph == 1)));
                NVQA_TRY(wgrad(c, dG, 4 * R, a.Hs[l] + (size_t)(q0 + (a.bridge && ph ? 1 : 0)) * B * R, R, 4 * R, R, K, c->G + w_h2h_of(c, l, ph == 1)));
                NVQA_TRY(colsum(c, dG, K, 4 * R, 4 * R, c->G + (ph ? c->lo.d_b_i2h[l] : c->lo.b_i2h[l]),
                                c->G + (ph ? c->lo.d_b_h2h[l] : c->lo.b_h2h[l])));
            }
        }
        if (!a.feats) { // this layer's slices of the decoder and the encoder segment, under the layers below / the lookup gradient
            NVQA_TRY(ae_comm_reduce(c, c->lo.d_w_i2h[l], c->lo.d_b_h2h[l] + 4 * (size_t)R - c->lo.d_w_i2h[l], 3 + l));
            NVQA_TRY(ae_comm_reduce(c, c->lo.w_i2h[l], c->lo.b_h2h[l] + 4 * (size_t)R - c->lo.w_i2h[l], 3 + l));
        }
        if (l > 0) { // d(h of layer l-1) through the inter-layer Dropout: the external term of layer l-1's chain
            const size_t n = (size_t)Q * B * R;
            hipLaunchKernelGGL(k_ae_drop<false>, dim3((unsigned)std::min<size_t>((n + 255) / 256, 4096)), dim3(256), 0, c->s, a.dX, a.dHx,
                               n, R, B, a.dstr, L, l, TE, 0, 0, dr, (unsigned short *)nullptr);
            NVQA_HIP(hipGetLastError());
        }
    }
    if (a.wp) { // the projection: dW_p = dx0^T f^ (K = B), db_p = colsum(dx0); dx0 = layer 0's d(input) rows of chain step 0
        const int I = d.I;
        ProfScope ps(c, PF_AE_WP_PROJ_BWD, 2.0 * B * E * (double)I);
        NVQA_TRY(wgrad(c, a.dX, E, a.feat, I, E, I, B, a.wp_g));
        NVQA_TRY(colsum(c, a.dX, B, E, E, a.wp_g + (size_t)E * I, nullptr));
        if (want_df) { // d(loss)/d(f^) = dx0 W_p (W_p [E x I]); its buffer on first use: a context that never asks pays nothing
            if (!a.dfeat) NVQA_TRY(ae_alloc(&a.dev, (void **)&a.dfeat, (size_t)B * I * 4, c->s));
            GemmArgs g = ae_args(a.dX, E, a.wp_x, I, B, I, E);
            const EpiStore e{a.dfeat, I, 0};
            AE_LAUNCH(AeCfgStepBwd, A_KC, B_NC, false, EpiStore, 0, g, e);
        }
        return 0;
    }
    if (a.bridge) return 0; // the frozen table has no gradient
    {   // lookup table: both token streams into one gradient (AE2: every chain row but the image's)
        ProfScope ps(c, PF_AE_EMB_BWD, 0, (double)Q * B * E * (a.ae2 ? 4 : 12));
        NVQA_HIP(hipMemsetAsync(c->G + c->lo.w_lk, 0, (size_t)Vp1 * E * 4, c->s));
        int nu = a.h_lk[0], nch = a.h_lk[1];
        const int nt = std::min(256, (E + 63) / 64 * 64);
        const int32_t *cu = nullptr, *cc = nullptr;
        if (a.lk_dev) { // nu / nch are on the device: grids of their upper bounds (nch <= nu + rows / chunk), the kernels cut themselves
            const int np = Q * B - (a.ae2 ? B : 0);
            nu = std::min(Vp1, np);
            nch = std::min(np, nu + np / NVQA_AE_LK_CHUNK);
            cu = a.lk_cnt;
            cc = a.lk_cnt + 1;
        }
        if (a.ae2)
            hipLaunchKernelGGL(k_ae2_lk_part, dim3(nch), dim3(nt), 0, c->s, a.lk_start, a.lk_pos, a.dX, E, a.lk_part, cc);
        else
            hipLaunchKernelGGL(k_ae_lk_part, dim3(nch), dim3(nt), 0, c->s, a.lk_start, a.lk_pos, a.X0, a.dX, B, a.D, E, T, dr, a.lk_part, cc);
        hipLaunchKernelGGL(k_ae_lk_sum, dim3(nu), dim3(nt), 0, c->s, a.lk_tok, a.lk_tc, a.lk_part, E, c->G + c->lo.w_lk, cu);
        NVQA_HIP(hipGetLastError());
    }
    NVQA_TRY(ae_comm_reduce(c, c->lo.w_lk, (size_t)Vp1 * E, 2));
    return 0;
}

// host side of a batch: tokens -> device, tmax, the criterion's n, and (training) the token -> rows index of the lookup
// gradient (ae_chain.h chain_index).  Weak-paired: enc_tokens -> etok; feats -> feat, L2-normalised over the n rows (the
// padding rows stay zero).  With `body` the features come from the extractor, which
// runs here, behind every check of the batch: its stream hands fc7o over by an event, the normalisation reads it straight into
// feat, and the extractor's next pass waits for that read.
static int ae_stage(const char *what, const int32_t *src, int n, int B, int D, int V, int32_t *dst, int *tmax)
{
    TokenFault bad;
    if (stage_tokens(src, n, B, D, V, dst, tmax, &bad)) return 0;
    set_error("ae: %s %d at (%d, %d) outside 0..%d", what, bad.value, (int)bad.row, bad.col, V);
    return -1;
}

// src [n x w] through the pinned h onto the device's [B x w], rows from n on zero
static int ae_stage_rows(nvqa_ctx *c, const float *src, size_t n, size_t w, float *h, float *dev)
{
    memcpy(h, src, n * w * 4);
    memset(h + n * w, 0, (c->d.B - n) * w * 4);
    NVQA_HIP(hipMemcpyAsync(dev, h, c->d.B * w * 4, hipMemcpyHostToDevice, c->s));
    return 0;
}

static int ae_upload(nvqa_ctx *c, const AeBatch &bt, bool index)
{
    AeState &a = *c->ae;
    const nvqa_dims &d = c->d;
    const int B = d.B, D = a.D, V = d.V, n = bt.n;
    const AeBody *body = bt.body;
    // the staging buffers may still feed the previous step's copies.  AE2_WP waits for those copies only, so that staging its
    // B x I features overlaps the previous step's kernels
    if (a.feats && a.staged_rec) NVQA_HIP(hipEventSynchronize(a.staged));
    else NVQA_HIP(hipStreamSynchronize(c->s));
    int tmax = 0, tmax_e = 0;
    NVQA_TRY(ae_stage("token", bt.tokens, n, B, D, V, a.h_tok, &tmax));
    if (tmax == 0) { set_error("ae: the batch holds no token (every row is null)"); return -1; }
    a.ncount = 0;
    for (int b = 0; b < n; ++b) a.ncount += criterion_count(a.h_tok + (size_t)b * D, D);
    if (a.feats) NVQA_TRY(ae_stage("enc_tokens", bt.enc_tokens, n, B, D, V, a.h_etok, &tmax_e));
    a.skip = a.bridge && bt.enc_state;
    a.tmax = tmax;
    a.te = encoder_steps(a.flags, tmax, tmax_e, a.skip);
    if (a.bridge && !a.skip && tmax_e == 0) { set_error("ae: enc_tokens holds no token (every row is null)"); return -1; }
    NVQA_HIP(hipMemcpyAsync(a.tok, a.h_tok, (size_t)B * D * 4, hipMemcpyHostToDevice, c->s));
    if (a.feats) {
        const size_t I = d.I;
        if (a.skip) NVQA_TRY(ae_stage_rows(c, bt.enc_state, n, 2 * (size_t)d.R, a.h_j, a.jbuf));
        NVQA_HIP(hipMemcpyAsync(a.etok, a.h_etok, (size_t)B * D * 4, hipMemcpyHostToDevice, c->s));
        if (body) {
            NVQA_HIP(hipEventRecord(a.staged, c->s));
            a.staged_rec = true;
            const float *fdev = nullptr;
            hipStream_t vs = nullptr;
            if (body->finetune)
                NVQA_TRY(nvqa_vgg_train_forward_raw_device(body->vgg, body->fn, body->images, n, body->S, body->xoff, body->yoff, body->dr, &fdev, &vs));
            else
                NVQA_TRY(nvqa_vgg_forward_raw_device(body->vgg, body->fn, body->images, n, body->S, body->xoff, body->yoff, body->dr, &fdev, &vs));
            if (!c->evStart) NVQA_HIP(hipEventCreateWithFlags(&c->evStart, hipEventDisableTiming)); // (nvqa_destroy releases it)
            NVQA_HIP(hipEventRecord(c->evStart, vs));
            NVQA_HIP(hipStreamWaitEvent(c->s, c->evStart, 0));
            if (n < B) NVQA_HIP(hipMemsetAsync(a.feat + (size_t)n * I, 0, (size_t)(B - n) * I * 4, c->s));
            {
                ProfScope ps(c, a.bridge ? PF_AE1WP_BRIDGE_FWD : PF_AE_WP_PROJ_FWD, 0, (double)n * I * 12);
                NVQA_TRY(l2norm_copy_launch(c->s, fdev, n, (int)I, a.feat));
            }
            NVQA_TRY(nvqa_vgg_features_taken(body->vgg, c->s));
        } else {
            NVQA_TRY(ae_stage_rows(c, bt.feats, n, I, a.h_feat, a.feat));
            NVQA_HIP(hipEventRecord(a.staged, c->s));
            a.staged_rec = true;
            ProfScope ps(c, a.bridge ? PF_AE1WP_BRIDGE_FWD : PF_AE_WP_PROJ_FWD, 0, (double)n * I * 12);
            NVQA_TRY(l2norm_rows_launch(c->s, a.feat, n, (int)I));
        }
    }
    a.img_live = a.ae2 && bt.images;
    if (a.img_live) NVQA_TRY(ae_stage_rows(c, bt.images, n, d.E, a.h_img, a.img));
    if (index) {
        const int NP = (a.te + tmax + 1 - (a.ae2 ? 1 : 0)) * B; // every chain row but AE2's image step
        int32_t *ut = a.h_lk + 2, *tc = ut + NP, *cs = tc + NP + 1, *pos = cs + NP + 1;
        chain_index(ae_chain(c), a.h_tok, a.h_tok, ut, tc, cs, pos, &a.h_lk[0], &a.h_lk[1]);
        const int nu = a.h_lk[0], nch = a.h_lk[1];
        a.lk_dev = false;
        NVQA_HIP(hipMemcpyAsync(a.lk_tok, ut, (size_t)nu * 4, hipMemcpyHostToDevice, c->s));
        NVQA_HIP(hipMemcpyAsync(a.lk_tc, tc, (size_t)(nu + 1) * 4, hipMemcpyHostToDevice, c->s));
        NVQA_HIP(hipMemcpyAsync(a.lk_start, cs, (size_t)(nch + 1) * 4, hipMemcpyHostToDevice, c->s));
        NVQA_HIP(hipMemcpyAsync(a.lk_pos, pos, (size_t)NP * 4, hipMemcpyHostToDevice, c->s));
    }
    return 0;
}

// (a data-parallel step: the sum over the ranks of loss_r n_r world / N, over world = the global batch's loss)
float ae_last_loss(const nvqa_ctx *c)
{
    if (!c->ae) return 0.f;
    return c->ae->loss_global ? c->h_dp_status[2] * (1.0f / (float)c->world) : *c->ae->h_loss;
}

// AE2_WP part of nvqa_init_params: W_p = uniform(lo, hi) from the seed, b_p = 0 (build_cnn, misc/net_utils.lua:38-40), and a
// fresh start of the projection's Adam
int ae_wp_init(nvqa_ctx *c, uint64_t seed, float lo, float hi)
{
    AeState &a = *c->ae;
    const size_t nw = (size_t)c->d.E * c->d.I, np = nw + c->d.E;
    std::vector<float> w(np, 0.f);
    for (size_t i = 0; i < nw; ++i) { // site 98: the flat vector's draw uses 99
        const float u = (float)(nvqa_hash32(seed, 0, 98u, i) >> 8) * (1.0f / 16777216.0f);
        w[i] = lo + (hi - lo) * u;
    }
    NVQA_HIP(hipStreamSynchronize(c->s));
    NVQA_HIP(hipMemcpy(a.wp_x, w.data(), np * 4, hipMemcpyHostToDevice));
    NVQA_HIP(hipMemset(a.wp_m, 0, np * 4));
    NVQA_HIP(hipMemset(a.wp_v, 0, np * 4));
    if (a.wp_vel) NVQA_HIP(hipMemset(a.wp_vel, 0, np * 4));
    a.wp_t = 0;
    return 0;
}

static int ae_check(nvqa_ctx *c)
{
    if (!c) { set_error("ctx is NULL"); return -1; }
    if (!is_ae(c->d) || !c->ae) {
        set_error("not an auto-encoder context (arch %d; NVQA_ARCH_AE1 = 3, NVQA_ARCH_AE2 = 4, NVQA_ARCH_AE2_WP = 5, NVQA_ARCH_AE1_WP = 6)", c->d.arch);
        return -1;
    }
    NVQA_HIP(hipSetDevice(c->device));
    return 0;
}

// the context's arch must be one of `allowed` (bits 1 << NVQA_ARCH_*): one arch, or AE_TEXT for the calls that carry no features
#define AE_ARCH(x) (1u << NVQA_ARCH_##x)
#define AE_TEXT (AE_ARCH(AE1) | AE_ARCH(AE2))
static int ae_check_arch(nvqa_ctx *c, const char *fn, unsigned allowed)
{
    NVQA_TRY(ae_check(c));
    const int arch = c->d.arch;
    if (allowed >> arch & 1u) return 0;
    if (allowed != AE_TEXT)
        set_error("%s: an NVQA_ARCH_%s context expected (arch %d)", fn,
                  allowed == AE_ARCH(AE2) ? "AE2" : (allowed == AE_ARCH(AE2_WP) ? "AE2_WP" : "AE1_WP"), arch);
    else if (arch == NVQA_ARCH_AE2_WP)
        set_error("%s: not available on a weak-paired auto-encoder context (NVQA_ARCH_AE2_WP: nvqa_ae_wp_step / nvqa_ae_wp_evaluate)", fn);
    else
        set_error("%s: not available on an arch1 weak-paired auto-encoder context (NVQA_ARCH_AE1_WP: nvqa_ae1_wp_step / nvqa_ae1_wp_evaluate)", fn);
    return -1;
}

// The data-parallel step's first exchange.  The ranks' criterion counts differ, and the mean of their means is not the global
// batch's mean: N = sum n_r is formed on the device, on the communication stream, under the forward pass.  No host ever sees
// another rank's count.  The communication stream is idle (the last step joined it), and nothing may read the old weight any
// more when k_ae_set_count overwrites it: the host-fed step knows that from ae_upload, which has drained the compute stream;
// the resident step (edge) drains nothing and makes the communication stream wait for the compute stream's position instead.
static int ae_dp_count(nvqa_ctx *c, bool edge)
{
    AeState &a = *c->ae;
    if (edge) {
        if (!a.step_ev) NVQA_HIP(hipEventCreateWithFlags(&a.step_ev, hipEventDisableTiming));
        NVQA_HIP(hipEventRecord(a.step_ev, c->s));
        NVQA_HIP(hipStreamWaitEvent(c->sc, a.step_ev, 0));
    }
    hipLaunchKernelGGL(k_ae_set_count, dim3(1), dim3(1), 0, c->sc, a.dpw, (float)a.ncount);
    NVQA_HIP(hipGetLastError());
    NVQA_TRY(ae_comm_count(c, a.dpw));
    hipLaunchKernelGGL(k_ae_rank_weight, dim3(1), dim3(1), 0, c->sc, a.dpw, (float)c->world);
    NVQA_HIP(hipGetLastError());
    NVQA_HIP(hipEventRecord(c->evComm, c->sc));
    a.dp_wait = true;
    return 0;
}

// every refusal that concerns the extractor, before anything is launched (the batch's own are ae_upload's, which run first there)
static int ae_check_body(nvqa_ctx *c, const AeBody &b, int n)
{
    if (!b.vgg) { set_error("%s: vgg is NULL", b.fn); return -1; }
    if (n < 1 || n > c->d.B) { set_error("%s: n = %d outside 1..B (%d)", b.fn, n, c->d.B); return -1; }
    int dev = 0, F = 0;
    nvqa_vgg_where(b.vgg, &dev, &F);
    if (F != c->d.I) { set_error("%s: extractor feature width %d != dims.I %d", b.fn, F, c->d.I); return -1; }
    if (dev != c->device) { set_error("%s: the extractor lives on device %d, the context on device %d", b.fn, dev, c->device); return -1; }
    return nvqa_vgg_check_raw(b.vgg, b.fn, b.images, n, b.S, b.xoff, b.yoff, b.dr);
}

// behind the forward pass of a training step: backward, the data-parallel join, and the route's counter (-1: none)
static int ae_train_tail(nvqa_ctx *c, const Drop &dr, bool want_df, int route)
{
    NVQA_TRY(ae_backward(c, dr, want_df));
    NVQA_TRY(ae_comm_join(c));
    c->have_grads = true;
    if (route >= 0) c->ae->routes[route] += 1;
    return 0;
}

static int ae_step_impl(nvqa_ctx *c, AeBatch bt, const nvqa_dropout *dropout, float *loss_out, float *dimages_out, float *dfeats_out)
{
    bt.n = c->d.B;
    if (bt.body) NVQA_TRY(ae_check_body(c, *bt.body, bt.n));
    const bool finetune = bt.body && bt.body->finetune;
    if (finetune) NVQA_TRY(nvqa_vgg_train_check_device(bt.body->vgg, bt.body->fn));
    if (!bt.tokens) { set_error("tokens is NULL"); return -1; }
    const Drop dr = ae_drop(dropout, true);
    NVQA_TRY(ae_upload(c, bt, !c->ae->feats));
    if (c->comm) NVQA_TRY(ae_dp_count(c, false));
    NVQA_TRY(ae_forward(c, dr, c->d.B, true));
    NVQA_TRY(ae_train_tail(c, dr, dfeats_out != nullptr || finetune, c->ae->feats ? -1 : 0));
    // fine-tuning: d f^ goes to the extractor on the device -- L2Normalize's backward and the body's backward on its stream
    if (finetune) NVQA_TRY(nvqa_vgg_backward_device(bt.body->vgg, bt.body->fn, c->ae->dfeat, bt.n, c->s));
    if (dfeats_out) {
        NVQA_HIP(hipMemcpyAsync(dfeats_out, c->ae->dfeat, (size_t)c->d.B * c->d.I * 4, hipMemcpyDeviceToHost, c->s));
        NVQA_HIP(hipStreamSynchronize(c->s));
    }
    if (dimages_out) // layer 0's d(input) of chain step 0 (the backward pass ends with layer 0)
        NVQA_HIP(hipMemcpyAsync(dimages_out, c->ae->dX, (size_t)c->d.B * c->d.E * 4, hipMemcpyDeviceToHost, c->s));
    if (loss_out || dimages_out) {
        NVQA_HIP(hipStreamSynchronize(c->s));
        if (loss_out) *loss_out = ae_last_loss(c);
    }
    return 0;
}

// evaluate mode on the batch in place (n valid rows): the teacher-forced loss and, on request, greedy decoding
static int ae_evaluate_run(nvqa_ctx *c, int32_t n, float *loss_out, int32_t *samples_out)
{
    AeState &a = *c->ae;
    NVQA_TRY(ae_forward(c, ae_drop(nullptr, false), n, false));
    if (samples_out) {
        // sample(): the encoder state is the one just computed (slot te); the decoder is fed START, then its own argmax
        for (int s = 0; s < a.D; ++s) {
            NVQA_TRY(ae_decode_step(c, s, a.cur, false));
            hipLaunchKernelGGL(k_ae_argmax, dim3(c->d.B), dim3(256), 0, c->s, a.logits + (size_t)s * c->d.B * a.ldl, a.ldl, c->d.V + 1,
                               a.D, s, a.cur, a.samples);
            NVQA_HIP(hipGetLastError());
        }
        NVQA_HIP(hipMemcpyAsync(samples_out, a.samples, (size_t)n * a.D * 4, hipMemcpyDeviceToHost, c->s));
    }
    NVQA_HIP(hipStreamSynchronize(c->s));
    if (loss_out) *loss_out = *a.h_loss;
    return 0;
}

static int ae_evaluate_impl(nvqa_ctx *c, const AeBatch &bt, float *loss_out, int32_t *samples_out)
{
    if (bt.body) NVQA_TRY(ae_check_body(c, *bt.body, bt.n));
    if (!bt.tokens) { set_error("tokens is NULL"); return -1; }
    if (bt.n < 1 || bt.n > c->d.B) { set_error("n = %d outside 1..B (%d)", bt.n, c->d.B); return -1; }
    NVQA_TRY(ae_upload(c, bt, false));
    return ae_evaluate_run(c, bt.n, loss_out, samples_out);
}

// ------------------------------------------------------------------------------------------------------------------
// the resident corpus: host side
// ------------------------------------------------------------------------------------------------------------------
// the launch plan of a batch of corpus rows from the host tables: tmax, te, the criterion's n.  Nothing is launched: every
// error of a resident step is raised here, before its first kernel and (data parallel) before its first collective.
static int ae_rows_plan(nvqa_ctx *c, const char *fn, int n, const int64_t *rows)
{
    AeState &a = *c->ae;
    if (!rows) { set_error("%s: rows is NULL", fn); return -1; }
    if (!a.corpus) { set_error("%s: no corpus is loaded (nvqa_ae_corpus_load comes first)", fn); return -1; }
    int tmax = 0, cnt = 0;
    for (int i = 0; i < n; ++i) {
        const int64_t r = rows[i];
        if (r < 0 || r >= a.corpus_rows) {
            set_error("%s: rows[%d] = %lld outside 0..%lld (the corpus holds %lld rows)", fn, i, (long long)r,
                      (long long)a.corpus_rows - 1, (long long)a.corpus_rows);
            return -1;
        }
        tmax = std::max(tmax, (int)a.row_last[r]);
        cnt += a.row_cnt[r];
    }
    if (tmax == 0) { set_error("ae: the batch holds no token (every row is null)"); return -1; }
    a.tmax = tmax;
    a.te = encoder_steps(a.flags, tmax, 0, false);
    a.skip = a.img_live = false; // (AE2: zero image rows, as the text script feeds)
    a.ncount = cnt;
    return 0;
}

// the batch of ae_rows_plan onto the device: the ids ride in the kernel arguments of the gather (NVQA_QARG_MAX per launch), so
// no staging buffer has to be waited for; index: the lookup gradient's token -> rows index, built from the gathered tokens
static int ae_rows_launch(nvqa_ctx *c, int n, const int64_t *rows, bool index)
{
    AeState &a = *c->ae;
    const int B = c->d.B, D = a.D, V = c->d.V;
    {
        ProfScope ps(c, PF_AE_EMB, 0, (double)B * D * 8);
        for (int b0 = 0; b0 < B; b0 += NVQA_QARG_MAX) {
            const int nb = std::min(NVQA_QARG_MAX, B - b0);
            QIdxArg ids;
            for (int k = 0; k < nb; ++k) ids.q[k] = b0 + k < n ? (int32_t)rows[b0 + k] : 0;
            hipLaunchKernelGGL(k_ae_gather_rows, dim3((unsigned)((nb * D + 255) / 256)), dim3(256), 0, c->s, (const int32_t *)a.corpus, ids,
                               b0, nb, n, D, a.tok);
        }
        NVQA_HIP(hipGetLastError());
    }
    if (!index) return 0;
    const int TE = a.te, Q = TE + a.tmax + 1, q_lo = a.ae2 ? 1 : 0, r_lo = q_lo * B, np = Q * B - r_lo;
    ProfScope ps(c, PF_AE_EMB_BWD, 0, (double)Q * (V + 2) * 16);
    NVQA_HIP(hipMemsetAsync(a.lk_hist, 0, (size_t)Q * (V + 2) * 4, c->s)); // every bin this step's kernels read, whatever the last step's Q was
    hipLaunchKernelGGL(k_ae_lk_hist, dim3((unsigned)((np + 255) / 256)), dim3(256), 0, c->s, ae_chain(c),
                       (const int32_t *)a.tok, r_lo, np, a.lk_hist);
    hipLaunchKernelGGL(k_ae_lk_prefix, dim3((unsigned)((V + 1 + 255) / 256)), dim3(256), 0, c->s, (const int32_t *)a.lk_hist, V, q_lo, Q,
                       a.lk_base, a.lk_tot);
    hipLaunchKernelGGL(k_ae_lk_scan, dim3(1), dim3(NVQA_AE_SCAN_NT), 0, c->s, V, a.lk_tot, a.lk_chb, a.lk_tok, a.lk_tc, a.lk_start,
                       a.lk_cnt);
    hipLaunchKernelGGL(k_ae_lk_rank, dim3((unsigned)(Q - q_lo), (unsigned)((B + 255) / 256)), dim3(256), 0, c->s, ae_chain(c),
                       (const int32_t *)a.tok, q_lo, (const int32_t *)a.lk_base, (const int32_t *)a.lk_tot, (const int32_t *)a.lk_chb,
                       a.lk_start, a.lk_pos);
    NVQA_HIP(hipGetLastError());
    a.lk_dev = true;
    return 0;
}


// ------------------------------------------------------------------------------------------------------------------
// decoding: nvqa_ae_sample / nvqa_ae_sample_rows (ae_decode.h)
// ------------------------------------------------------------------------------------------------------------------
struct AeSample { int mode = 0, K = 1; float T = 1.f; uint64_t seed = 0, step = 0; };

// every refusal of the two calls but those of the batch itself (tokens, rows), before anything is launched
static int ae_sample_check(nvqa_ctx *c, const char *fn, int n, const nvqa_sample_opts *opts, bool images, const int32_t *seq_out,
                           AeSample *o)
{
    NVQA_TRY(ae_check(c));
    if (c->ae->feats) {
        set_error("%s: not available on a weak-paired auto-encoder context (arch %d): nvqa_ae_wp_evaluate / nvqa_ae1_wp_evaluate decode "
                  "greedily", fn, c->d.arch);
        return -1;
    }
    const nvqa_dims &d = c->d;
    if (!seq_out) { set_error("%s: seq_out is NULL", fn); return -1; }
    if (n < 1 || n > d.B) { set_error("%s: n = %d outside 1..B (%d)", fn, n, d.B); return -1; }
    if (images && d.arch != NVQA_ARCH_AE2) { set_error("%s: images on an NVQA_ARCH_AE1 context (the text auto-encoder takes none)", fn); return -1; }
    if (opts) {
        o->mode = opts->mode; o->K = opts->beam_size; o->T = opts->temperature; o->seed = opts->seed; o->step = opts->step;
    }
    if (o->mode < 0 || o->mode > 2) { set_error("%s: mode %d outside 0..2 (argmax, multinomial, beam)", fn, o->mode); return -1; }
    if (o->mode == 1 && !(o->T > 0.f && std::isfinite(o->T))) { set_error("%s: temperature %g must be finite and > 0", fn, (double)o->T); return -1; }
    if (o->mode == 2) {
        if (o->K < 1 || o->K > NVQA_AE_BEAM_MAX) { set_error("%s: beam_size %d outside 1..%d", fn, o->K, NVQA_AE_BEAM_MAX); return -1; }
        if (o->K > d.V + 1) { set_error("%s: beam_size %d above the V + 1 = %d classes", fn, o->K, d.V + 1); return -1; }
        if ((int64_t)n * o->K > d.B) { set_error("%s: n beam_size = %d x %d decoder rows exceed B (%d)", fn, n, o->K, d.B); return -1; }
    } else o->K = 1;
    if (d.V + 1 > NVQA_AE_SEL_NT * 4 * NVQA_AE_SEL_MAXV4) {
        set_error("%s: V + 1 = %d exceeds the %d columns the selection kernels hold in registers", fn, d.V + 1, NVQA_AE_SEL_NT * 4 * NVQA_AE_SEL_MAXV4);
        return -1;
    }
    if (d.R % 4) { set_error("%s: R = %d is not a multiple of 4 (the state gather moves 16 bytes a thread)", fn, d.R); return -1; }
    return 0;
}

static int ae_sample_alloc(nvqa_ctx *c, bool beam)
{
    AeState &a = *c->ae;
    const size_t B = c->d.B, D = a.D, R = c->d.R;
    if (a.slp && (!beam || a.bm_bp)) return 0;
    if (!a.slp) AE_ALLOC(a.slp, B * D);
    if (beam && !a.bm_bp) {
        for (int l = 0; l < c->d.L; ++l) {
            AE_ALLOC(a.bm_h[l], B * R);
            AE_ALLOC(a.bm_c[l], B * R);
        }
        AE_ALLOC(a.bm_tk, D * B);
        AE_ALLOC(a.bm_lp, D * B);
        AE_ALLOC(a.bm_score, B);
        AE_ALLOC(a.bm_fin, B);
        AE_ALLOC(a.bm_csc, B * NVQA_AE_BEAM_MAX);
        AE_ALLOC(a.bm_clp, B * NVQA_AE_BEAM_MAX);
        AE_ALLOC(a.bm_cc, B * NVQA_AE_BEAM_MAX);
        AE_ALLOC(a.bm_bp, D * B);
    }
    NVQA_HIP(hipDeviceSynchronize()); // (the zero fills ran on the null stream)
    return 0;
}

// the selection kernels by the float4s a thread holds: 1 (V + 1 <= 1024), 4 (<= 4096), 16 (<= 16384)
#define AE_SEL_DISPATCH(KERNEL, grid, ...)                                                                                    \
    do {                                                                                                                      \
        if (Vp1 <= NVQA_AE_SEL_NT * 4) hipLaunchKernelGGL(KERNEL<1>, grid, dim3(NVQA_AE_SEL_NT), 0, c->s, __VA_ARGS__);       \
        else if (Vp1 <= NVQA_AE_SEL_NT * 16) hipLaunchKernelGGL(KERNEL<4>, grid, dim3(NVQA_AE_SEL_NT), 0, c->s, __VA_ARGS__); \
        else hipLaunchKernelGGL(KERNEL<NVQA_AE_SEL_MAXV4>, grid, dim3(NVQA_AE_SEL_NT), 0, c->s, __VA_ARGS__);                 \
    } while (0)

// the batch in place (n rows; tmax / te set): the encoder (ae_run_encoder: the state the decoder starts from has nvqa_ae_evaluate's
// bits), then D decoder steps fed START and their own picks.  Nothing synchronises inside the loop; one copy per output at the end.
static int ae_sample_run(nvqa_ctx *c, int32_t n, const AeSample &o, int32_t *seq_out, float *logprobs_out)
{
    AeState &a = *c->ae;
    const nvqa_dims &d = c->d;
    const int B = d.B, R = d.R, L = d.L, D = a.D, TE = a.te, Vp1 = d.V + 1, K = o.K, nK = n * K;
    const bool beam = o.mode == 2;
    NVQA_TRY(ae_wproj_images(c));
    NVQA_TRY(ae_run_encoder(c, ae_drop(nullptr, false)));
    const dim3 ggrid((unsigned)std::min<size_t>(((size_t)nK * (R / 4) + 255) / 256, 1024));
    if (beam) { // sentence i's final encoder state (slot te, row i) to its K decoder rows
        for (int l = 0; l < L; ++l)
            hipLaunchKernelGGL(k_ae_beam_gather, ggrid, dim3(256), 0, c->s, (const float *)(a.Hs[l] + (size_t)TE * B * R),
                               (const float *)(a.Cs[l] + (size_t)TE * B * R), a.bm_h[l], a.bm_c[l], (const int32_t *)nullptr, K, nK, R / 4);
        NVQA_HIP(hipGetLastError());
    }
    for (int s = 0; s < D; ++s) {
        const int q = TE + s;
        const float *lg = a.logits + (size_t)s * B * a.ldl;
        NVQA_TRY(ae_decode_step(c, s, a.cur, beam));
        if (!beam) {
            AE_SEL_DISPATCH(k_ae_select, dim3(n), lg, a.ldl, Vp1, D, s, o.mode, o.T, o.seed, o.step, a.cur, a.samples, a.slp);
            NVQA_HIP(hipGetLastError());
            continue;
        }
        AE_SEL_DISPATCH(k_ae_beam_rows, dim3(nK), lg, a.ldl, Vp1, s, K, (const float *)a.bm_score, (const int32_t *)a.bm_fin, a.bm_csc,
                        a.bm_clp, a.bm_cc);
        hipLaunchKernelGGL(k_ae_beam_merge, dim3(n), dim3(64), 0, c->s, K, s, B, Vp1, (const float *)a.bm_csc, (const float *)a.bm_clp,
                           (const int32_t *)a.bm_cc, a.bm_score, a.bm_fin, a.cur, a.bm_bp, a.bm_tk, a.bm_lp);
        if (s + 1 < D) // the survivors' states: slot q + 1 (just written) through the back-pointers into the buffers step q + 1 reads
            for (int l = 0; l < L; ++l)
                hipLaunchKernelGGL(k_ae_beam_gather, ggrid, dim3(256), 0, c->s, (const float *)(a.Hs[l] + (size_t)(q + 1) * B * R),
                                   (const float *)(a.Cs[l] + (size_t)(q + 1) * B * R), a.bm_h[l], a.bm_c[l],
                                   (const int32_t *)(a.bm_bp + (size_t)s * B), K, nK, R / 4);
        NVQA_HIP(hipGetLastError());
    }
    if (beam) {
        hipLaunchKernelGGL(k_ae_beam_out, dim3((n + 63) / 64), dim3(64), 0, c->s, n, K, D, B, (const int32_t *)a.bm_bp,
                           (const int32_t *)a.bm_tk, (const float *)a.bm_lp, a.samples, a.slp);
        NVQA_HIP(hipGetLastError());
    }
    NVQA_HIP(hipMemcpyAsync(seq_out, a.samples, (size_t)n * D * 4, hipMemcpyDeviceToHost, c->s));
    if (logprobs_out) NVQA_HIP(hipMemcpyAsync(logprobs_out, a.slp, (size_t)n * D * 4, hipMemcpyDeviceToHost, c->s));
    NVQA_HIP(hipStreamSynchronize(c->s));
    return 0;
}

} // namespace nvqa

extern "C" int nvqa_ae_sample(nvqa_ctx *c, int32_t n, const float *images, const int32_t *tokens, const nvqa_sample_opts *opts,
                              int32_t *seq_out, float *logprobs_out)
{
    AeSample o;
    NVQA_TRY(ae_sample_check(c, "nvqa_ae_sample", n, opts, images != nullptr, seq_out, &o));
    if (!tokens) { set_error("nvqa_ae_sample: tokens is NULL"); return -1; }
    NVQA_TRY(ae_sample_alloc(c, o.mode == 2));
    NVQA_TRY(ae_upload(c, AeBatch{.n = n, .tokens = tokens, .images = images}, false));
    return ae_sample_run(c, n, o, seq_out, logprobs_out);
}

extern "C" int nvqa_ae_sample_rows(nvqa_ctx *c, int32_t n, const int64_t *rows, const nvqa_sample_opts *opts, int32_t *seq_out,
                                   float *logprobs_out)
{
    AeSample o;
    NVQA_TRY(ae_sample_check(c, "nvqa_ae_sample_rows", n, opts, false, seq_out, &o));
    NVQA_TRY(ae_rows_plan(c, "nvqa_ae_sample_rows", n, rows));
    NVQA_TRY(ae_sample_alloc(c, o.mode == 2));
    NVQA_TRY(ae_rows_launch(c, n, rows, false));
    return ae_sample_run(c, n, o, seq_out, logprobs_out);
}

extern "C" int nvqa_ae_corpus_load(nvqa_ctx *c, int64_t n_rows, const int32_t *tokens)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_corpus_load", AE_TEXT));
    if (!tokens) { set_error("nvqa_ae_corpus_load: tokens is NULL"); return -1; }
    AeState &a = *c->ae;
    const int D = a.D, V = c->d.V;
    if (n_rows < 1 || n_rows > INT32_MAX) { set_error("nvqa_ae_corpus_load: n_rows = %lld outside 1..2^31-1", (long long)n_rows); return -1; }
    if (D >= 65535) { set_error("nvqa_ae_corpus_load: seq_length %d does not fit the per-row host tables", D); return -1; }
    int tmax = 0;
    TokenFault bad;
    if (!stage_tokens(tokens, n_rows, n_rows, D, V, nullptr, &tmax, &bad)) {
        set_error("nvqa_ae_corpus_load: token %d at (row %lld, column %d) outside 0..%d", bad.value, (long long)bad.row, bad.col, V);
        return -1;
    }
    std::vector<uint16_t> last((size_t)n_rows), cnt((size_t)n_rows);
    for (int64_t r = 0; r < n_rows; ++r) {
        last[(size_t)r] = (uint16_t)row_last(tokens + (size_t)r * D, D);
        cnt[(size_t)r] = (uint16_t)criterion_count(tokens + (size_t)r * D, D);
    }
    if (!a.lk_cnt) { // the index build's scratch, on first use
        const size_t W = (size_t)V + 2;
        AE_ALLOC(a.lk_hist, (size_t)a.QM * W);
        AE_ALLOC(a.lk_base, (size_t)a.QM * W);
        AE_ALLOC(a.lk_tot, W);
        AE_ALLOC(a.lk_chb, W);
        AE_ALLOC(a.lk_cnt, 2);
    }
    const size_t bytes = (size_t)n_rows * D * 4;
    int32_t *dev = nullptr;
    hipError_t e = hipMalloc((void **)&dev, bytes);
    if (e != hipSuccess) {
        set_error("nvqa_ae_corpus_load: hipMalloc of %zu bytes for %lld rows failed: %s", bytes, (long long)n_rows, hipGetErrorString(e));
        return -1;
    }
    e = hipMemcpy(dev, tokens, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipStreamSynchronize(c->s); // steps in flight still gather from the old corpus
    if (e != hipSuccess) {
        (void)hipFree(dev);
        set_error("nvqa_ae_corpus_load: copying %zu bytes to the device failed: %s", bytes, hipGetErrorString(e));
        return -1;
    }
    if (a.corpus) (void)hipFree(a.corpus);
    a.corpus = dev;
    a.corpus_rows = n_rows;
    a.row_last.swap(last);
    a.row_cnt.swap(cnt);
    return 0;
}

extern "C" int nvqa_ae_step_rows(nvqa_ctx *c, const int64_t *rows, const nvqa_dropout *dropout, float *loss_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_step_rows", AE_TEXT));
    const Drop dr = ae_drop(dropout, true);
    NVQA_TRY(ae_rows_plan(c, "nvqa_ae_step_rows", c->d.B, rows));
    if (c->comm) NVQA_TRY(ae_dp_count(c, true));
    NVQA_TRY(ae_rows_launch(c, c->d.B, rows, true));
    NVQA_TRY(ae_forward(c, dr, c->d.B, true));
    NVQA_TRY(ae_train_tail(c, dr, false, 1));
    if (loss_out) {
        NVQA_HIP(hipStreamSynchronize(c->s));
        *loss_out = ae_last_loss(c);
    }
    return 0;
}

extern "C" int nvqa_ae_evaluate_rows(nvqa_ctx *c, int32_t n, const int64_t *rows, float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_evaluate_rows", AE_TEXT));
    if (n < 1 || n > c->d.B) { set_error("n = %d outside 1..B (%d)", n, c->d.B); return -1; }
    NVQA_TRY(ae_rows_plan(c, "nvqa_ae_evaluate_rows", n, rows));
    NVQA_TRY(ae_rows_launch(c, n, rows, false));
    return ae_evaluate_run(c, n, loss_out, samples_out);
}

extern "C" int nvqa_ae_step_routes(const nvqa_ctx *c, int64_t out[2])
{
    if (!c || !out) { set_error("NULL argument"); return -1; }
    if (!c->ae || (c->d.arch != NVQA_ARCH_AE1 && c->d.arch != NVQA_ARCH_AE2)) {
        set_error("nvqa_ae_step_routes: an NVQA_ARCH_AE1 / NVQA_ARCH_AE2 context expected (arch %d)", c->d.arch);
        return -1;
    }
    out[0] = c->ae->routes[0];
    out[1] = c->ae->routes[1];
    return 0;
}

// The bf16 operand mode of the AE1 / AE2 step.  A switch of its own: nvqa_set_precision(ctx, 1) stays
// refused on every auto-encoder context.
extern "C" int nvqa_ae_set_precision(nvqa_ctx *c, int bf16)
{
    if (!c) { set_error("ctx is NULL"); return -1; }
    if (!is_ae(c->d) || !c->ae) {
        set_error("nvqa_ae_set_precision: an NVQA_ARCH_AE1 / NVQA_ARCH_AE2 context expected (arch %d); the VQA step's switch is nvqa_set_precision", c->d.arch);
        return -1;
    }
    if (c->ae->feats) {
        set_error("nvqa_ae_set_precision: not available on a weak-paired auto-encoder context (arch %d): at the scripts' batch sizes "
                  "the step is bound by its launches, and the image projection and the state bridge stay f32", c->d.arch);
        return -1;
    }
    if (bf16 != 0 && bf16 != 1) { set_error("nvqa_ae_set_precision: precision must be 0 (f32) or 1 (bf16 operands)"); return -1; }
    AeState &a = *c->ae;
    if (bf16) {
        NVQA_HIP(hipSetDevice(c->device));
        if (c->d.R % 8 == 0 && !a.G16) { // the images of the projection group, on first use: an f32-only context never holds them
            const size_t B = c->d.B, R = c->d.R, Vp1 = (size_t)c->d.V + 1, rows = ((size_t)a.D + 1) * B;
            a.ld16 = (int)((Vp1 + 7) / 8 * 8);
            AE_ALLOC(a.Htd16, rows * R);
            AE_ALLOC(a.Wp16, Vp1 * R);
            AE_ALLOC(a.WpT16, R * a.ld16);
            AE_ALLOC(a.rowlse, rows);
            AE_ALLOC(a.rowtgt, rows);
            AE_ALLOC(a.G16, rows * a.ld16);
            NVQA_HIP(hipDeviceSynchronize()); // (the zero fills ran on the null stream)
        }
    }
    a.bf16 = bf16 != 0;
    a.p16 = a.bf16 && a.G16 != nullptr;
    return 0;
}

// AE2: images = NULL (the text script's zero image rows)
extern "C" int nvqa_ae_step(nvqa_ctx *c, const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_step", AE_TEXT));
    return ae_step_impl(c, AeBatch{.tokens = tokens}, dropout, loss_out, nullptr, nullptr);
}

extern "C" int nvqa_ae_evaluate(nvqa_ctx *c, int32_t n, const int32_t *tokens, float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_evaluate", AE_TEXT));
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens}, loss_out, samples_out);
}

extern "C" int nvqa_ae_step_images(nvqa_ctx *c, const float *images, const int32_t *tokens, const nvqa_dropout *dropout,
                                   float *loss_out, float *dimages_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_step_images", AE_ARCH(AE2)));
    return ae_step_impl(c, AeBatch{.tokens = tokens, .images = images}, dropout, loss_out, dimages_out, nullptr);
}

extern "C" int nvqa_ae_evaluate_images(nvqa_ctx *c, int32_t n, const float *images, const int32_t *tokens, float *loss_out,
                                       int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_evaluate_images", AE_ARCH(AE2)));
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens, .images = images}, loss_out, samples_out);
}

extern "C" int nvqa_ae_wp_step(nvqa_ctx *c, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                               const nvqa_dropout *dropout, float *loss_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_step", AE_ARCH(AE2_WP)));
    if (!feats) { set_error("nvqa_ae_wp_step: feats is NULL"); return -1; }
    return ae_step_impl(c, AeBatch{.tokens = tokens, .feats = feats, .enc_tokens = enc_tokens}, dropout, loss_out, nullptr, nullptr);
}

extern "C" int nvqa_ae_wp_evaluate(nvqa_ctx *c, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                                   float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_evaluate", AE_ARCH(AE2_WP)));
    if (!feats) { set_error("nvqa_ae_wp_evaluate: feats is NULL"); return -1; }
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens, .feats = feats, .enc_tokens = enc_tokens}, loss_out, samples_out);
}

extern "C" int nvqa_ae1_wp_step(nvqa_ctx *c, const float *feats, const int32_t *enc_tokens, const float *enc_state,
                                const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_step", AE_ARCH(AE1_WP)));
    if (!feats) { set_error("nvqa_ae1_wp_step: feats is NULL"); return -1; }
    if ((enc_tokens != nullptr) == (enc_state != nullptr)) {
        set_error("nvqa_ae1_wp_step: exactly one of enc_tokens and enc_state must be given");
        return -1;
    }
    return ae_step_impl(c, AeBatch{.tokens = tokens, .feats = feats, .enc_tokens = enc_tokens, .enc_state = enc_state}, dropout, loss_out,
                        nullptr, dfeats_out);
}

extern "C" int nvqa_ae1_wp_evaluate(nvqa_ctx *c, int32_t n, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                                    float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_evaluate", AE_ARCH(AE1_WP)));
    if (!feats || !enc_tokens) { set_error("nvqa_ae1_wp_evaluate: feats or enc_tokens is NULL"); return -1; }
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens, .feats = feats, .enc_tokens = enc_tokens}, loss_out, samples_out);
}

// nvqa_ae_wp_step with d(loss)/d(f^) = dx0 W_p returned (one more product): what nvqa_vgg16_backward(..., 1) takes
extern "C" int nvqa_ae_wp_step_dfeats(nvqa_ctx *c, const float *feats, const int32_t *enc_tokens, const int32_t *tokens,
                                      const nvqa_dropout *dropout, float *loss_out, float *dfeats_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_step_dfeats", AE_ARCH(AE2_WP)));
    if (!feats || !dfeats_out) { set_error("nvqa_ae_wp_step_dfeats: feats or dfeats_out is NULL"); return -1; }
    return ae_step_impl(c, AeBatch{.tokens = tokens, .feats = feats, .enc_tokens = enc_tokens}, dropout, loss_out, nullptr, dfeats_out);
}

// ---- the weak-paired steps with the VGG-16 body in the loop ----
extern "C" int nvqa_ae_wp_step_images(nvqa_ctx *c, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                      const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                      const nvqa_dropout *dropout, float *loss_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_step_images", AE_ARCH(AE2_WP)));
    const AeBody body{vgg, "nvqa_ae_wp_step_images", images_u8, S, xoff, yoff, body_dropout};
    return ae_step_impl(c, AeBatch{.tokens = tokens, .enc_tokens = enc_tokens, .body = &body}, dropout, loss_out, nullptr, nullptr);
}

// the same step with the body fine-tuning (section 9.11): training forward, the step, L2Normalize's backward, the body's backward
extern "C" int nvqa_ae_wp_step_images_finetune(nvqa_ctx *c, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                               const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                               const nvqa_dropout *dropout, float *loss_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_step_images_finetune", AE_ARCH(AE2_WP)));
    const AeBody body{vgg, "nvqa_ae_wp_step_images_finetune", images_u8, S, xoff, yoff, body_dropout, true};
    return ae_step_impl(c, AeBatch{.tokens = tokens, .enc_tokens = enc_tokens, .body = &body}, dropout, loss_out, nullptr, nullptr);
}

extern "C" int nvqa_ae_wp_evaluate_images(nvqa_ctx *c, nvqa_vgg *vgg, int32_t n, const uint8_t *images_u8, int S, int xoff, int yoff,
                                          const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                          float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_evaluate_images", AE_ARCH(AE2_WP)));
    const AeBody body{vgg, "nvqa_ae_wp_evaluate_images", images_u8, S, xoff, yoff, body_dropout};
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens, .enc_tokens = enc_tokens, .body = &body}, loss_out, samples_out);
}

extern "C" int nvqa_ae1_wp_step_images(nvqa_ctx *c, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                       const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const float *enc_state,
                                       const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_step_images", AE_ARCH(AE1_WP)));
    if ((enc_tokens != nullptr) == (enc_state != nullptr)) {
        set_error("nvqa_ae1_wp_step_images: exactly one of enc_tokens and enc_state must be given");
        return -1;
    }
    const AeBody body{vgg, "nvqa_ae1_wp_step_images", images_u8, S, xoff, yoff, body_dropout};
    return ae_step_impl(c, AeBatch{.tokens = tokens, .enc_tokens = enc_tokens, .enc_state = enc_state, .body = &body}, dropout, loss_out,
                        nullptr, dfeats_out);
}

extern "C" int nvqa_ae1_wp_step_images_finetune(nvqa_ctx *c, nvqa_vgg *vgg, const uint8_t *images_u8, int S, int xoff, int yoff,
                                                const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const float *enc_state,
                                                const int32_t *tokens, const nvqa_dropout *dropout, float *loss_out, float *dfeats_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_step_images_finetune", AE_ARCH(AE1_WP)));
    if ((enc_tokens != nullptr) == (enc_state != nullptr)) {
        set_error("nvqa_ae1_wp_step_images_finetune: exactly one of enc_tokens and enc_state must be given");
        return -1;
    }
    const AeBody body{vgg, "nvqa_ae1_wp_step_images_finetune", images_u8, S, xoff, yoff, body_dropout, true};
    return ae_step_impl(c, AeBatch{.tokens = tokens, .enc_tokens = enc_tokens, .enc_state = enc_state, .body = &body}, dropout, loss_out,
                        nullptr, dfeats_out);
}

extern "C" int nvqa_ae1_wp_evaluate_images(nvqa_ctx *c, nvqa_vgg *vgg, int32_t n, const uint8_t *images_u8, int S, int xoff, int yoff,
                                           const nvqa_dropout *body_dropout, const int32_t *enc_tokens, const int32_t *tokens,
                                           float *loss_out, int32_t *samples_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_evaluate_images", AE_ARCH(AE1_WP)));
    if (!enc_tokens) { set_error("nvqa_ae1_wp_evaluate_images: enc_tokens is NULL"); return -1; }
    const AeBody body{vgg, "nvqa_ae1_wp_evaluate_images", images_u8, S, xoff, yoff, body_dropout};
    return ae_evaluate_impl(c, AeBatch{.n = n, .tokens = tokens, .enc_tokens = enc_tokens, .body = &body}, loss_out, samples_out);
}

// the evaluate-mode encoder alone: [c_T | h_T] of the state slot te, joined by the bridge's prep kernel
extern "C" int nvqa_ae1_wp_encode(nvqa_ctx *c, int32_t n, const int32_t *enc_tokens, float *state_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_encode", AE_ARCH(AE1_WP)));
    if (!enc_tokens || !state_out) { set_error("nvqa_ae1_wp_encode: NULL argument"); return -1; }
    if (n < 1 || n > c->d.B) { set_error("n = %d outside 1..B (%d)", n, c->d.B); return -1; }
    AeState &a = *c->ae;
    const int B = c->d.B, D = a.D, V = c->d.V, R = c->d.R, I = c->d.I;
    NVQA_HIP(hipStreamSynchronize(c->s));
    int te = 0;
    NVQA_TRY(ae_stage("enc_tokens", enc_tokens, n, B, D, V, a.h_etok, &te));
    if (te == 0) { set_error("ae: enc_tokens holds no token (every row is null)"); return -1; }
    a.te = encoder_steps(a.flags, 0, te, false);
    a.skip = false;
    NVQA_HIP(hipMemcpyAsync(a.etok, a.h_etok, (size_t)B * D * 4, hipMemcpyHostToDevice, c->s));
    const Drop dr = ae_drop(nullptr, false);
    NVQA_TRY(ae_run_encoder(c, dr));
    const size_t sl = (size_t)te * B * R;
    hipLaunchKernelGGL(k_ae1wp_bridge_prep, dim3((unsigned)std::min<size_t>(((size_t)B * (2 * R + I) + 255) / 256, 2048)), dim3(256), 0,
                       c->s, (const float *)(a.Cs[0] + sl), (const float *)(a.Hs[0] + sl), a.jbuf, (const float *)a.feat, B, R, I, dr,
                       a.qd, a.vd);
    NVQA_HIP(hipGetLastError());
    NVQA_HIP(hipMemcpyAsync(state_out, a.jbuf, (size_t)n * 2 * R * 4, hipMemcpyDeviceToHost, c->s));
    NVQA_HIP(hipStreamSynchronize(c->s));
    return 0;
}

extern "C" int nvqa_ae1_wp_set_lookup(nvqa_ctx *c, const float *w)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_set_lookup", AE_ARCH(AE1_WP)));
    if (!w) { set_error("NULL argument"); return -1; }
    NVQA_HIP(hipStreamSynchronize(c->s));
    NVQA_HIP(hipMemcpy(c->P + c->lo.w_lk, w, ((size_t)c->d.V + 1) * c->d.E * 4, hipMemcpyHostToDevice));
    return 0;
}

extern "C" int nvqa_ae1_wp_get_lookup(nvqa_ctx *c, float *w_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae1_wp_get_lookup", AE_ARCH(AE1_WP)));
    if (!w_out) { set_error("NULL argument"); return -1; }
    NVQA_HIP(hipStreamSynchronize(c->s));
    NVQA_HIP(hipMemcpy(w_out, c->P + c->lo.w_lk, ((size_t)c->d.V + 1) * c->d.E * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nvqa_ae_wp_set_projection(nvqa_ctx *c, const float *w, const float *b)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_set_projection", AE_ARCH(AE2_WP)));
    if (!w || !b) { set_error("NULL argument"); return -1; }
    AeState &a = *c->ae;
    const size_t nw = (size_t)c->d.E * c->d.I;
    NVQA_HIP(hipStreamSynchronize(c->s));
    NVQA_HIP(hipMemcpy(a.wp_x, w, nw * 4, hipMemcpyHostToDevice));
    NVQA_HIP(hipMemcpy(a.wp_x + nw, b, (size_t)c->d.E * 4, hipMemcpyHostToDevice));
    return 0;
}

static int ae_wp_copy_out(nvqa_ctx *c, const float *src, float *w_out, float *b_out)
{
    if (!w_out || !b_out) { set_error("NULL argument"); return -1; }
    const size_t nw = (size_t)c->d.E * c->d.I;
    NVQA_HIP(hipStreamSynchronize(c->s));
    NVQA_HIP(hipMemcpy(w_out, src, nw * 4, hipMemcpyDeviceToHost));
    NVQA_HIP(hipMemcpy(b_out, src + nw, (size_t)c->d.E * 4, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int nvqa_ae_wp_get_projection(nvqa_ctx *c, float *w_out, float *b_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_get_projection", AE_ARCH(AE2_WP)));
    return ae_wp_copy_out(c, c->ae->wp_x, w_out, b_out);
}

extern "C" int nvqa_ae_wp_get_projection_grads(nvqa_ctx *c, float *w_out, float *b_out)
{
    NVQA_TRY(ae_check_arch(c, "nvqa_ae_wp_get_projection_grads", AE_ARCH(AE2_WP)));
    if (!c->have_grads) { set_error("nvqa_ae_wp_get_projection_grads before any nvqa_ae_wp_step"); return -1; }
    return ae_wp_copy_out(c, c->ae->wp_g, w_out, b_out);
}

// the per-workgroup partial sums of an update's statistics -> {sqrt(sum x^2), count}
static int optim_read_stats(nvqa_ctx *c, const double *part, int NB, float stats_out[2])
{
    std::vector<double> h(2 * NB);
    NVQA_HIP(hipMemcpyAsync(h.data(), part, 2 * NB * sizeof(double), hipMemcpyDeviceToHost, c->s));
    NVQA_HIP(hipStreamSynchronize(c->s));
    double sq = 0, cnt = 0;
    for (int b = 0; b < NB; ++b) { sq += h[2 * b]; cnt += h[2 * b + 1]; }
    stats_out[0] = (float)sqrt(sq);
    stats_out[1] = (float)cnt;
    return 0;
}

// Adam's bias-corrected rate at step t (optim_updates.lua:99-102)
static float adam_step_size(float lr, float beta1, float beta2, int64_t t)
{
    return (float)(lr * sqrt(1.0 - pow((double)beta2, (double)t)) / (1.0 - pow((double)beta1, (double)t)));
}

static int ae_wp_projection_rule(nvqa_ctx *c, const char *fn, int rule, float lr, float alpha, float beta, float eps, float wd,
                                 float clamp, float stats_out[2])
{
    NVQA_TRY(ae_check_arch(c, fn, AE_ARCH(AE2_WP)));
    if (rule != NVQA_OPT_SGD && rule != NVQA_OPT_SGDM && rule != NVQA_OPT_ADAM) {
        set_error("%s: rule %d is not one of -cnn_optim's (NVQA_OPT_SGD, NVQA_OPT_SGDM, NVQA_OPT_ADAM)", fn, rule);
        return -1;
    }
    if (!c->have_grads) { set_error("%s before any nvqa_ae_wp_step", fn); return -1; }
    AeState &a = *c->ae;
    const size_t nw = (size_t)c->d.E * c->d.I, n = nw + c->d.E;
    const int NB = 1024;
    if (rule == NVQA_OPT_SGDM && !a.wp_vel) NVQA_TRY(ae_alloc(&a.dev, (void **)&a.wp_vel, n * 4, c->s)); // (zeroed in stream order)
    RuleArgs r = {lr, alpha, beta, eps, 0.f};
    if (rule == NVQA_OPT_ADAM) r.step = adam_step_size(lr, alpha, beta, ++a.wp_t);
    double *part = stats_out ? a.wp_part : (double *)nullptr;
    const float *g = a.wp_g;
    if (rule == NVQA_OPT_ADAM) {
        ProfScope ps(c, PF_ADAM, 0, 28.0 * n);
        hipLaunchKernelGGL(k_ae_wp_optim<NVQA_OPT_ADAM>, dim3(NB), dim3(256), 0, c->s, a.wp_x, a.wp_m, a.wp_v, g, n, nw, r, wd, clamp, part);
    } else if (rule == NVQA_OPT_SGDM) {
        ProfScope ps(c, PF_RMSPROP, 0, 20.0 * n);
        hipLaunchKernelGGL(k_ae_wp_optim<NVQA_OPT_SGDM>, dim3(NB), dim3(256), 0, c->s, a.wp_x, a.wp_vel, (float *)nullptr, g, n, nw, r, wd, clamp, part);
    } else {
        ProfScope ps(c, PF_RMSPROP, 0, 12.0 * n);
        hipLaunchKernelGGL(k_ae_wp_optim<NVQA_OPT_SGD>, dim3(NB), dim3(256), 0, c->s, a.wp_x, (float *)nullptr, (float *)nullptr, g, n, nw, r, wd, clamp, part);
    }
    NVQA_HIP(hipGetLastError());
    return stats_out ? optim_read_stats(c, a.wp_part, NB, stats_out) : 0;
}

extern "C" int nvqa_ae_wp_projection_adam(nvqa_ctx *c, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                                          float stats_out[2])
{
    return ae_wp_projection_rule(c, "nvqa_ae_wp_projection_adam", NVQA_OPT_ADAM, lr, beta1, beta2, eps, wd, clamp, stats_out);
}

extern "C" int nvqa_ae_wp_projection_update(nvqa_ctx *c, int rule, float lr, float alpha, float beta, float eps, float wd,
                                            float clamp, float stats_out[2])
{
    return ae_wp_projection_rule(c, "nvqa_ae_wp_projection_update", rule, lr, alpha, beta, eps, wd, clamp, stats_out);
}

template <int RULE>
static void optim_launch(nvqa_ctx *c, const OptimArgs &a, int NB, int group)
{
    ProfScope ps(c, group, 0, (12.0 + 8.0 * RuleState<RULE>::n) * a.n);
    hipLaunchKernelGGL(k_optim<RULE>, dim3(NB), dim3(256), 0, c->s, a);
}

// Every rule of misc/optim_updates.lua over the flat vector; AE2_WP: [encoder | decoder] only (the reference's params; the frozen
// lookup is left out of parameters()).  State: SGD none; SGDM, SGDMOM, ADAGRAD one buffer each (c->opt_state, allocated and zeroed
// on first use); RMSPROP the buffer of nvqa_rmsprop_update (c->M2); ADAM adam_m / adam_v / adam_t.
static int optim_update(nvqa_ctx *c, const char *fn, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                        float stats_out[2])
{
    if (!c) { set_error("ctx is NULL"); return -1; }
    if (rule < NVQA_OPT_SGD || rule > NVQA_OPT_ADAM) { set_error("%s: unknown rule %d (NVQA_OPT_SGD = 0 .. NVQA_OPT_ADAM = 5)", fn, rule); return -1; }
    if (!c->have_grads) { set_error("%s before any step", fn); return -1; }
    NVQA_HIP(hipSetDevice(c->device));
    const size_t n = c->lo.total;
    const int NB = 1024;
    OptimArgs a = {};
    if (rule == NVQA_OPT_ADAM) {
        if (!c->adam_v) { // adam_v is set last: after a failed allocation the next call starts here again, and nothing leaks
            if (!c->adam_m) NVQA_HIP(hipMalloc((void **)&c->adam_m, n * 4 + 16));
            NVQA_HIP(hipMalloc((void **)&c->adam_v, n * 4 + 16));
            NVQA_HIP(hipMemsetAsync(c->adam_m, 0, n * 4, c->s));
            NVQA_HIP(hipMemsetAsync(c->adam_v, 0, n * 4, c->s));
            c->adam_t = 0;
        }
        c->adam_t += 1;
        a.m = c->adam_m; a.v = c->adam_v;
    } else if (rule == NVQA_OPT_RMSPROP) {
        a.m = c->M2;
    } else if (rule != NVQA_OPT_SGD) {
        float *&st = c->opt_state[rule - NVQA_OPT_SGDM];
        if (!st) {
            NVQA_HIP(hipMalloc((void **)&st, n * 4 + 16));
            NVQA_HIP(hipMemsetAsync(st, 0, n * 4, c->s));
        }
        a.m = st;
    }
    // (adam_part: the statistics' partial sums of every rule, not Adam's alone, so allocated apart from adam_m / adam_v)
    if (stats_out && !c->adam_part) NVQA_HIP(hipMalloc((void **)&c->adam_part, 2 * NB * sizeof(double)));
    a.x = c->P; a.g = c->G;
    a.n = c->d.arch == NVQA_ARCH_AE2_WP ? c->lo.seg[0] + c->lo.seg[1] : n;
    a.seg0 = c->lo.seg[0]; a.seg1 = c->lo.seg[0] + c->lo.seg[1];
    const float inv_world = 1.0f / (float)c->world;
    for (int i = 0; i < 3; ++i) a.gs[i] = c->gscale[i] * inv_world;
    a.r.lr = lr; a.r.b1 = alpha; a.r.b2 = beta; a.r.eps = eps; a.wd = wd; a.clamp = clamp;
    if (rule == NVQA_OPT_ADAM) a.r.step = adam_step_size(lr, alpha, beta, c->adam_t);
    a.skip = c->comm ? nullptr : c->pf_sticky;
    a.dp_skip = c->comm ? c->dp_status + c->dp_slot : nullptr;
    a.h_dp = c->comm ? c->h_dp_status : nullptr;
    a.dp_next = c->comm ? c->dp_status + (c->dp_slot ^ 1) : nullptr;
    a.part = stats_out ? c->adam_part : nullptr;
    switch (rule) {
    case NVQA_OPT_SGD: optim_launch<NVQA_OPT_SGD>(c, a, NB, PF_RMSPROP); break;
    case NVQA_OPT_SGDM: optim_launch<NVQA_OPT_SGDM>(c, a, NB, PF_RMSPROP); break;
    case NVQA_OPT_SGDMOM: optim_launch<NVQA_OPT_SGDMOM>(c, a, NB, PF_RMSPROP); break;
    case NVQA_OPT_ADAGRAD: optim_launch<NVQA_OPT_ADAGRAD>(c, a, NB, PF_RMSPROP); break;
    case NVQA_OPT_RMSPROP: optim_launch<NVQA_OPT_RMSPROP>(c, a, NB, PF_RMSPROP); break;
    default: optim_launch<NVQA_OPT_ADAM>(c, a, NB, PF_ADAM); break;
    }
    NVQA_HIP(hipGetLastError());
    if (c->comm) c->dp_clean[c->dp_slot ^ 1] = true;
    return stats_out ? optim_read_stats(c, c->adam_part, NB, stats_out) : 0;
}

extern "C" int nvqa_adam_update(nvqa_ctx *c, float lr, float beta1, float beta2, float eps, float wd, float clamp,
                                float stats_out[2])
{
    return optim_update(c, "nvqa_adam_update", NVQA_OPT_ADAM, lr, beta1, beta2, eps, wd, clamp, stats_out);
}

extern "C" int nvqa_optim_update(nvqa_ctx *c, int rule, float lr, float alpha, float beta, float eps, float wd, float clamp,
                                 float stats_out[2])
{
    return optim_update(c, "nvqa_optim_update", rule, lr, alpha, beta, eps, wd, clamp, stats_out);
}
