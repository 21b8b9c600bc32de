"""Text auto-encoder, CPU side: the float64 yardstick's criterion, the data loader's wrap-around, and the export table."""
import numpy as np
import pytest

import ae_ref_torch as ref


def test_criterion_targets_by_hand():
    V = 9
    tok = np.array([[3, 4, 5, 6],    # full length: 4 words, then END at s = D
                    [7, 0, 0, 0],    # length 1
                    [2, 8, 0, 0]],   # padded tail
                   np.int32)
    tg, n = ref.criterion_targets(tok, V)
    assert tg == {(0, 0): 2, (1, 0): 3, (2, 0): 4, (3, 0): 5, (4, 0): V,
                  (0, 1): 6, (1, 1): V,
                  (0, 2): 1, (1, 2): 7, (2, 2): V}
    assert n == (4 + 1) + (1 + 1) + (2 + 1)
    assert ref.tmax_of(tok) == 4
    # tmax < D: every row shorter than the buffer
    short = np.array([[1, 2, 0, 0, 0], [3, 0, 0, 0, 0]], np.int32)
    tg, n = ref.criterion_targets(short, V)
    assert ref.tmax_of(short) == 2 and n == 3 + 2
    assert max(s for s, _ in tg) == 2  # no target beyond tmax: the decoder runs tmax + 1 steps


def test_torch_model_loss_is_mean_over_criterion_positions():
    dims = (3, 4, 9, 4, 4, 1)
    lo = ref.layout(*dims)
    rng = np.random.default_rng(0)
    p = rng.uniform(-0.08, 0.08, lo["_total"])
    tok = np.array([[3, 4, 5, 6], [7, 0, 0, 0], [2, 8, 0, 0]], np.int32)
    out = ref.forward(dims, p, tok, want_grads=True)
    logp = out["logits"] - np.log(np.exp(out["logits"]).sum(2, keepdims=True))
    tg, n = ref.criterion_targets(tok, dims[2])
    assert out["n"] == n
    assert abs(out["loss"] + sum(logp[s, b, c] for (s, b), c in tg.items()) / n) < 1e-12
    assert out["grads"].shape == (lo["_total"],) and np.abs(out["grads"]).max() > 0


def test_get_batch_wraps_like_the_reference(pkg):
    data = np.arange(1, 11, dtype=np.int32).reshape(5, 2)  # rows 1..5, row k = [2k-1, 2k]
    ld = pkg.ae.DataLoader(labels={"train": data})
    b, info = ld.get_batch("train", 2)
    assert b.tolist() == [[1, 2], [3, 4]] and not info["wrapped"] and info["it_pos_now"] == 3
    b, info = ld.get_batch("train", 2)
    assert b.tolist() == [[5, 6], [7, 8]] and info["it_pos_now"] == 5
    b, info = ld.get_batch("train", 2)   # iterator AT the last row: the whole batch from the start, row 5 is skipped
    assert b.tolist() == [[1, 2], [3, 4]] and info["wrapped"] and info["it_pos_now"] == 1
    ld.iterators["train"] = 4            # rows 4, 5, then row 1; the iterator goes back to 1 ...
    b, info = ld.get_batch("train", 3)
    assert b.tolist() == [[7, 8], [9, 10], [1, 2]] and info["wrapped"] and info["it_pos_now"] == 1
    b, _ = ld.get_batch("train", 2)      # ... so row 1 repeats
    assert b.tolist() == [[1, 2], [3, 4]]


def test_decode_sequence_stops_at_end(pkg):
    words = {"1": "a", "2": "b", "3": "c"}
    assert pkg.ae.decode_sequence(words, [[1, 2, 4, 3], [3, 0, 1, 1]], end_token=4) == ["a b", "c"]


def test_export_table_round_trips_with_init_shapes(pkg, tmp_path):
    """the table export_for_vqa writes (here from a plain vector, no device) has the shapes init_from_autoencoder checks"""
    B, D, V, E, R, L = 2, 3, 7, 4, 8, 2
    lo = ref.layout(B, D, V, E, R, L)
    x = np.arange(lo["_total"], dtype=np.float32)

    class FakeCtx:
        def get_params(self):
            return x

        def segments(self):
            return (lo["_seg0"], lo["_seg1"], lo["_seg2"])

    tr = pkg.ae.AETrainer.__new__(pkg.ae.AETrainer)
    tr.dims, tr.ctx = pkg.binding.Dims(3, B, D, V, E, R, L, 0, 0, 0), FakeCtx()
    path = str(tmp_path / "ae.t7")
    tr.export_for_vqa(path)
    t = pkg.t7.load(path)
    assert t["layout"] == pkg.t7.LAYOUT_MARK
    assert np.asarray(t["lookup"]).shape == (E, V + 1)
    assert np.array_equal(np.asarray(t["lookup"]).T.ravel(), x[lo["w_lk"][0]:])
    assert np.array_equal(np.asarray(t["encoder"]), x[:lo["_seg0"]])
    # the arch1 VQA encoder of the same E, R, L has exactly this many values
    d1 = pkg.binding.Dims(1, B, D, V, E, R, L, 8, 8, 4)
    assert np.asarray(t["encoder"]).size == sum(4 * R * ((E if l == 0 else R) + R + 2) for l in range(L))
    assert d1.E == E


def test_ae_trainer_rejects_other_archs(pkg):
    with pytest.raises(ValueError):
        pkg.ae.AETrainer(pkg.binding.Dims(1, 2, 3, 4, 4, 4, 1, 4, 4, 4))
