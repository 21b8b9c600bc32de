"""The arithmetic of csrc/dx0_split.h, emulated on the CPU: d(layer-0 input) dX = dG W with every f32 value as three bf16
pieces (round-to-nearest-even: hi = bf16(x), mid = bf16(x - hi), lo = bf16(x - hi - mid)) and every f32 product as SIX
bf16 x bf16 terms summed into one f32 accumulator in the kernel's order -- lo hi, mid mid, hi lo, mid hi, hi mid, hi hi
(piece of dG x piece of W) -- K = 2048 in ascending chunks of 32, no split-K.  Operands shaped like the step's: dG
log-normal x 1e-3, W uniform in +-0.08 (the initialisation range), N = 200, 256 rows.  Against the f64 product the
six-term form must stay within 1.5 x of the f32 chain's L2-relative and 4 x of its max-relative error, the margins of
tests/test_wgrad_split_numerics.py (measured here: 0.43 x and 0.41 x -- the chain rounds after every one of its 2048
additions per output, the six-term form once per term and chunk; three terms: 5.7 x and 4.5 x).  What the hardware does inside one MFMA's K = 32 sum is measured by
tests/test_gpu_dx0_split.py."""
import torch

from split_emul import err as _err, mm, six as _six, split as _split

M, N, K, CHUNK = 256, 200, 2048, 32


def _mm(terms):
    return mm(terms, K, CHUNK, k_major=False)


def _chain(A, W):
    """The f32 fmaf chain over ascending k (each product exact in f64, one f32 rounding per addition)."""
    acc = torch.zeros(M, N, dtype=torch.float64)
    for k in range(K):
        acc = (acc + A[:, k:k + 1].double() * W[k:k + 1].double()).float().double()
    return acc.float()


def _operands(seed=0):
    torch.manual_seed(seed)
    A = (torch.randn(M, K) * torch.exp(torch.randn(M, K)) * 1e-3).float()
    W = ((torch.rand(K, N) * 2 - 1) * 0.08).float()
    return A, W


def test_pieces_of_the_weights_reassemble_them_exactly():
    _, W = _operands()
    h, m, l = _split(W)
    assert torch.equal(h + m + l, W)
    assert torch.equal(h.double() + m.double() + l.double(), W.double())


def test_six_terms_in_the_kernels_order_match_the_f32_chain():
    A, W = _operands()
    ref = A.double() @ W.double()
    m32, l32 = _err(_chain(A, W), ref)
    m6, l6 = _err(_mm(_six(A, W)), ref)
    print(f"f32 chain max {m32:.3g} L2 {l32:.3g}; six terms max {m6:.3g} L2 {l6:.3g} ({m6 / m32:.2f} x, {l6 / l32:.2f} x)")
    assert l6 <= 1.5 * l32 and m6 <= 4.0 * m32


def test_three_terms_would_not_do():
    """hi mid, mid hi, hi hi alone drop the 2^-16 terms and miss the L2 margin the six-term form is held to: that is why the
    kernel pays for six."""
    A, W = _operands()
    ref = A.double() @ W.double()
    m32, l32 = _err(_chain(A, W), ref)
    (ah, am, _), (wh, wm, _) = _split(A), _split(W)
    m3, l3 = _err(_mm([(ah, wm), (am, wh), (ah, wh)]), ref)
    print(f"three terms max {m3:.3g} L2 {l3:.3g} ({m3 / m32:.1f} x, {l3 / l32:.1f} x)")
    assert l3 > 1.5 * l32
