"""The arithmetic of csrc/wgrad_split.h, emulated on the CPU: an f32 value as three bf16 pieces (round-to-nearest-even:
hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)), an f32 product as SIX bf16 x bf16 terms summed into one f32
accumulator in the kernel's order -- lo hi, mid mid, hi lo, mid hi, hi mid, hi hi -- K in chunks.  On operands shaped like
the step's (dG log-normal x 1e-3, the other operand 2 tanh x Bernoulli(0.5) like Dropout(h); K = 13312) the six-term form
must stay within 1.5 x of the f32 chain's L2-relative and 4 x of its max-relative error against the f64 product (measured:
1.08 x and 2.2 x), and the three-term form (hi mid, mid hi, hi hi) must be worse than 5 x (measured 17 x): that is why
the kernel pays for six.  What the hardware does inside one MFMA's K = 32 sum is measured by tests/test_gpu_wgrad_split.py."""
import torch

from split_emul import bf as _bf, err as _err, mm, six as _six, split as _split

K, M, N, CHUNK = 13312, 512, 200, 512


def _mm(terms, k_total):
    return mm(terms, k_total, CHUNK, k_major=True)


def _three(A, B):
    (ah, am, _), (bh, bm, _) = _split(A), _split(B)
    return [(ah, bm), (am, bh), (ah, bh)]


def _operands(seed=0):
    torch.manual_seed(seed)
    A = (torch.randn(K, M) * torch.exp(torch.randn(K, M)) * 1e-3).float()
    B = (torch.tanh(torch.randn(K, N)) * (torch.rand(K, N) < 0.5) * 2).float()
    return A, B


def test_three_pieces_reassemble_the_f32_value_exactly():
    """Every f32 value whose pieces are normal numbers (below |x| ~ 2^-109 = 1.5e-33 a piece can be subnormal and may be
    flushed: an absolute error under 1e-35, no gradient lives there)."""
    A, _ = _operands()
    x = torch.cat([A.flatten()[:100000], torch.tensor([0.0, -0.0, 1.0, -1.0, 3.0e38, 1e-30, 1.17549435e-38, 2.5e-33, 1.0 + 2.0 ** -23,
                                                       1.0 - 2.0 ** -24, 255.99998, 16777215.0])])
    h, m, l = _split(x)
    assert torch.equal((h.double() + m.double() + l.double()), x.double())
    assert torch.equal(h + m + l, x)


def test_six_terms_match_the_f32_chain_three_do_not():
    A, B = _operands()
    ref = A.double().T @ B.double()
    m32, l32 = _err(_mm([(A, B)], K), ref)
    m6, l6 = _err(_mm(_six(A, B), K), ref)
    m3, l3 = _err(_mm(_three(A, B), K), ref)
    print(f"f32 chain max {m32:.3g} L2 {l32:.3g}; six terms max {m6:.3g} L2 {l6:.3g} ({m6 / m32:.2f} x, {l6 / l32:.2f} x); "
          f"three terms max {m3:.3g} L2 {l3:.3g} ({m3 / m32:.1f} x, {l3 / l32:.1f} x)")
    assert l6 <= 1.5 * l32 and m6 <= 4.0 * m32
    assert l3 > 5.0 * l32 and m3 > 5.0 * m32


def test_rows_with_subnormal_or_zero_low_pieces_exact_zeros_and_equal_large_values():
    """Rows of K whose lo piece vanishes or is subnormal, exact zeros (dropout), and a row of equal large values: the
    same bounds against the f32 chain on the same operands."""
    A, B = _operands(1)
    k = 2048
    A, B = A[:k].clone(), B[:k].clone()
    A[0:64] = _bf(A[0:64])                                   # mid = lo = 0
    h, m, _ = _split(A[64:128])
    A[64:128] = h + m                                        # lo = 0
    A[128:192] = (A[128:192] * 2.0 ** -100).float()          # x ~ 1e-33: lo ~ 2^-16 x is subnormal in bf16 / f32
    A[192:256] = 0.0                                         # exact zeros in one operand ...
    B[256:320] = 0.0                                         # ... and in the other
    A[320] = 3.0e4                                           # one row of equal large values, against
    B[320] = 1.9990234                                       # equal values of 11 significand bits
    h, m, l = _split(A[128:192])
    assert (l != 0).any() and (l.abs()[l != 0] < 1.1754944e-38).any()  # the subnormal case is really there
    ref = A.double().T @ B.double()
    m32, l32 = _err(_mm([(A, B)], k), ref)
    m6, l6 = _err(_mm(_six(A, B), k), ref)
    print(f"f32 chain max {m32:.3g} L2 {l32:.3g}; six terms max {m6:.3g} L2 {l6:.3g}")
    assert l6 <= 1.5 * l32 and m6 <= 4.0 * m32
    # the large row alone: one product per output, no cancellation -> the six terms are within two f32 ulps of it
    one = _mm(_six(A[320:321], B[320:321]), 1).double()
    exact = A[320:321].double().T @ B[320:321].double()
    assert float(((one - exact).abs() / exact.abs()).max()) <= 2.0 ** -22
