"""The arithmetic of csrc/kmajor_bf16.h, emulated on the CPU for tests/test_wgrad_split_numerics.py and
tests/test_dx0_split_numerics.py: an f32 value as three bf16 pieces (round-to-nearest-even: hi = bf16(x), mid = bf16(x - hi),
lo = bf16(x - hi - mid)), an f32 product as SIX bf16 x bf16 terms summed into one f32 accumulator in the kernels' order --
lo hi, mid mid, hi lo, mid hi, hi mid, hi hi -- K in chunks."""
import torch


def bf(x):
    return x.to(torch.bfloat16).to(torch.float32)  # round-to-nearest-even


def split(x):
    h = bf(x)
    r = x - h
    m = bf(r)
    return h, m, bf(r - m)


def six(A, B):
    (ah, am, al), (bh, bm, bl) = split(A), split(B)
    return [(al, bh), (am, bm), (ah, bl), (am, bh), (ah, bm), (ah, bh)]  # the kernels' order, smallest first


def mm(terms, k_total, chunk, k_major):
    """One f32 accumulator, K in chunks, the terms of a chunk in the order given.  k_major: the pairs are ([K][M], [K][N]) and
    the product is A^T B (the weight gradients); otherwise ([M][K], [K][N]) and it is A B (d(input))."""
    a0, b0 = terms[0]
    acc = torch.zeros(a0.shape[1] if k_major else a0.shape[0], b0.shape[1])
    for k in range(0, k_total, chunk):
        for a, b in terms:
            acc += a[k:k + chunk].T @ b[k:k + chunk] if k_major else a[:, k:k + chunk] @ b[k:k + chunk]
    return acc


def err(C, ref):
    d = C.double() - ref
    return float(d.abs().max() / ref.abs().max()), float(d.norm() / ref.norm())
