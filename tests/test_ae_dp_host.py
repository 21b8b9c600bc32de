"""Data-parallel text auto-encoder training, CPU side: AETrainer's seeds per rank, its comm_init, the log line, and the data
loader's rank-disjoint batches.  The context is a stand-in that records what the trainer asks of the library."""
import numpy as np
import pytest


class FakeCtx:
    def __init__(self, dims, device=0):
        self.dims, self.calls = dims, []

    def init_params(self, seed, lo, hi):
        self.calls.append(("init_params", seed, lo, hi))

    def ae_set_precision(self, bf16):
        self.calls.append(("ae_set_precision", bf16))

    def ae_comm_init(self, rank, world, comm_id):
        self.calls.append(("ae_comm_init", rank, world, bytes(comm_id)))

    def ae_step(self, tokens, dr):
        self.calls.append(("ae_step", int(dr.mode), int(dr.seed), int(dr.step)))
        return 2.5

    def adam_update(self, *a, stats=False):
        return (7.0, 3)


@pytest.fixture()
def fake_ctx(pkg, monkeypatch):
    monkeypatch.setattr(pkg.binding, "Context", FakeCtx)
    return pkg


@pytest.mark.parametrize("rank", [0, 1, 5])
def test_trainer_seeds_per_rank(fake_ctx, rank):
    pkg = fake_ctx
    tr = pkg.ae.AETrainer(pkg.binding.Dims(3, 4, 5, 9, 8, 8, 1, 0, 0, 0), seed=123, rank=rank)
    assert tr.ctx.calls[0] == ("init_params", 123, -0.08, 0.08)  # the parameter seed is common to all ranks
    assert tr.dropout_seed == 123 + 1000 * rank and tr.rank == rank and tr.world == 1
    cid = bytes(range(128))
    with pytest.raises(ValueError):
        tr.comm_init(rank + 1, 8, cid)
    tr.comm_init(rank, 8, cid)
    assert tr.ctx.calls[-1] == ("ae_comm_init", rank, 8, cid) and tr.world == 8
    out = [tr.train_step(np.ones((4, 5), np.int32)) for _ in range(2)]
    steps = [c for c in tr.ctx.calls if c[0] == "ae_step"]
    assert steps == [("ae_step", 1, 123 + 1000 * rank, 1), ("ae_step", 1, 123 + 1000 * rank, 2)]
    # the line is built from what the library returns, which with a communicator are the global values on every rank
    assert out[0][3] == "iter 1: loss: 2.500 | # updates:    3 | paramsNorm: 7.0000"


def test_default_rank_keeps_the_single_gpu_seeds(fake_ctx):
    pkg = fake_ctx
    tr = pkg.ae.AETrainer(pkg.binding.Dims(4, 4, 5, 9, 8, 8, 1, 0, 0, 0), seed=9, drop_prob=0.0)
    tr.train_step(np.ones((4, 5), np.int32))
    assert tr.dropout_seed == 9 and tr.ctx.calls[-1] == ("ae_step", 0, 9, 1)


def test_loader_draws_rank_disjoint_batches(pkg):
    data = np.arange(1, 23, dtype=np.int32).reshape(11, 2)  # rows 1..11
    world, bs = 2, 2
    one = pkg.ae.DataLoader(labels={"train": data})
    ranks = [pkg.ae.DataLoader(labels={"train": data}, rank=r, world=world) for r in range(world)]
    for _ in range(4):  # the third stride wraps (rows 9..11 then row 1), the fourth starts from row 1 again
        want, wb = one.get_batch("train", bs * world)
        got = [ld.get_batch("train", bs) for ld in ranks]
        assert np.array_equal(np.concatenate([g[0] for g in got]), want)  # disjoint, and their union is the global batch
        assert all(g[1] == wb for g in got)                              # every rank wraps in the same iteration
    assert wb["it_pos_now"] == 5
    with pytest.raises(ValueError):
        pkg.ae.DataLoader(labels={"train": data}, rank=2, world=2)
    # WeakPairedDataLoader keeps DataLoader's single-process walk
    wp = pkg.ae.WeakPairedDataLoader({"train": data}, {"train": np.zeros((11, 4), np.float32)})
    lab, feats, _ = wp.get_batch("train", 3)
    assert lab.tolist() == data[:3].tolist() and feats.shape == (3, 4)


def test_eval_split_walks_the_same_rows_on_every_rank(fake_ctx):
    """evaluation is rank-local and ignores the rank stride: every rank sees the split's rows in the single-process order"""
    pkg = fake_ctx
    data = np.arange(1, 25, dtype=np.int32).reshape(12, 2) % 9 + 1
    seen = []
    for r in range(2):
        tr = pkg.ae.AETrainer(pkg.binding.Dims(3, 4, 2, 9, 8, 8, 1, 0, 0, 0), rank=r)
        rows = []
        tr.ctx.ae_evaluate = lambda batch, samples=False, rows=rows: (rows.append(batch.copy()) or 1.0, np.ones_like(batch))
        loader = pkg.ae.DataLoader(labels={"val": data}, ix_to_word={str(i): f"w{i}" for i in range(1, 10)}, rank=r, world=2)
        loss, preds = tr.eval_split(loader, "val", val_sentences_use=8)
        assert loss == 1.0 and len(preds) == 8
        seen.append(np.concatenate(rows))
    assert np.array_equal(seen[0], data[:8]) and np.array_equal(seen[1], data[:8])
