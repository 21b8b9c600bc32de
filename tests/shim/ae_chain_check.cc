// ae_chain_check.cc -- prints what novel-vqa_amd/csrc/ae_chain.h makes of one batch, for tests/test_ae_chain_host.py (built there
// with g++ and the host sanitizers).  stdin: flags B D V n skip has_enc has_direct, tokens [n x D], then enc_tokens [n x D] if
// has_enc, then direct [B] if has_direct.  The batch is staged as ae_upload stages it; an invalid value ends the run with "bad".
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "ae_chain.h"

using namespace nvqa;

static void line(const char *name, const int32_t *v, int n)
{
    printf("%s", name);
    for (int i = 0; i < n; ++i) printf(" %d", v[i]);
    printf("\n");
}

static std::vector<int32_t> read_ints(size_t n)
{
    std::vector<int32_t> v(n);
    for (auto &x : v)
        if (scanf("%d", &x) != 1) { fprintf(stderr, "short input\n"); exit(3); }
    return v;
}

int main()
{
    const std::vector<int32_t> h = read_ints(8);
    const int flags = h[0], B = h[1], D = h[2], V = h[3], n = h[4], skip = h[5], has_enc = h[6], has_direct = h[7];
    const std::vector<int32_t> src = read_ints((size_t)n * D), esrc = read_ints(has_enc ? (size_t)n * D : 0);
    const std::vector<int32_t> direct = read_ints(has_direct ? B : 0);
    std::vector<int32_t> tok((size_t)B * D), etok((size_t)B * D);
    int tmax = 0, tmax_e = 0;
    TokenFault bad;
    if (!stage_tokens(src.data(), n, B, D, V, tok.data(), &tmax, &bad)) {
        printf("bad tokens %d %lld %d\n", bad.value, (long long)bad.row, bad.col);
        return 2;
    }
    if ((flags & AE_CHAIN_ENC) && !stage_tokens(has_enc ? esrc.data() : nullptr, n, B, D, V, etok.data(), &tmax_e, &bad)) {
        printf("bad enc_tokens %d %lld %d\n", bad.value, (long long)bad.row, bad.col);
        return 2;
    }
    const AeChain ch{B, D, V, encoder_steps(flags, tmax, tmax_e, skip != 0), tmax + 1, flags};
    const int32_t *enc = flags & AE_CHAIN_ENC ? etok.data() : tok.data();
    printf("tmax %d te %d\n", tmax, ch.te);
    line("staged", tok.data(), B * D);
    std::vector<int32_t> row(B);
    for (int q = 0; q < ch.te + ch.nd; ++q) {
        for (int b = 0; b < B; ++b) row[b] = chain_token(ch, enc, tok.data(), nullptr, q, b);
        line("chain", row.data(), B);
        if (!has_direct) continue;
        for (int b = 0; b < B; ++b) row[b] = chain_token(ch, enc, tok.data(), direct.data(), q, b);
        line("direct", row.data(), B);
    }
    const int NP = (ch.te + ch.nd - (flags & AE_CHAIN_AE2 ? 1 : 0)) * B;
    std::vector<int32_t> lk_tok(NP), lk_tc(NP + 1), lk_start(NP + 1), lk_pos(NP);
    int32_t nu = 0, nch = 0;
    chain_index(ch, enc, tok.data(), lk_tok.data(), lk_tc.data(), lk_start.data(), lk_pos.data(), &nu, &nch);
    printf("nu %d nch %d\n", nu, nch);
    line("lk_tok", lk_tok.data(), nu);
    line("lk_tc", lk_tc.data(), nu + 1);
    line("lk_start", lk_start.data(), nch + 1);
    line("lk_pos", lk_pos.data(), NP);
    for (int b = 0; b < B; ++b) { // row b: last, count, then the target of every decoder step s = 0 .. D
        const int32_t *t = tok.data() + (size_t)b * D;
        std::vector<int32_t> out = {row_last(t, D), criterion_count(t, D)};
        for (int s = 0; s <= D; ++s) out.push_back(criterion_target(t, s, D, V));
        line("row", out.data(), (int)out.size());
    }
    return 0;
}
