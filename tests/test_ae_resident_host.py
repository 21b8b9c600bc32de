"""The resident corpus, CPU side: DataLoader.corpus() and get_rows() name exactly the rows get_batch returns -- wrap, rank
stride, iterator reset -- and AETrainer routes train / eval_split through the row calls once load_corpus ran.  The context is a
stand-in that records what the trainer asks of the library."""
import numpy as np
import pytest

D = 3


def split(n, base):
    """n distinct rows: row i holds base + i in every column"""
    return np.repeat(np.arange(base, base + n, dtype=np.int32)[:, None], D, axis=1)


# split sizes against the batch (4): a multiple of it, one short of a multiple, smaller than the batch
SIZES = [8, 11, 3]


@pytest.mark.parametrize("rank_stride", [True, False])
@pytest.mark.parametrize("world", [1, 3])
@pytest.mark.parametrize("n", SIZES)
def test_get_rows_names_what_get_batch_returns(pkg, n, world, rank_stride):
    bs = 4
    labels = {"train": split(n, 1), "val": split(5, 100)}
    for rank in range(world):
        a = pkg.ae.DataLoader(labels=labels, rank=rank, world=world)
        b = pkg.ae.DataLoader(labels=labels, rank=rank, world=world)
        corpus, first = b.corpus()
        wraps = 0
        for _ in range(9):  # several wraps at every size
            want, wb = a.get_batch("train", bs, rank_stride=rank_stride)
            rows, gb = b.get_rows("train", bs, rank_stride=rank_stride)
            assert rows.dtype == np.int64 and rows.ndim == 1
            assert np.array_equal(corpus[rows], want), (rows, want)
            assert gb == wb
            assert a.iterators == b.iterators
            wraps += wb["wrapped"]
        assert wraps >= 2
        # the two calls move one iterator: alternating them walks the split as either alone does
        c = pkg.ae.DataLoader(labels=labels, rank=rank, world=world)
        a.reset_iterator("train")
        for k in range(6):
            want, wb = a.get_batch("train", bs, rank_stride=rank_stride)
            if k % 2:
                got, gb = c.get_batch("train", bs, rank_stride=rank_stride)
            else:
                rows, gb = c.get_rows("train", bs, rank_stride=rank_stride)
                got = c.corpus()[0][rows]
            assert np.array_equal(got, want) and gb == wb and a.iterators == c.iterators


def test_corpus_offsets(pkg):
    tr, va, te = split(7, 1), split(4, 50), split(5, 80)
    for labels in ({"train": tr}, {"val": va, "train": tr}, {"test": te, "val": va, "train": tr}):
        ld = pkg.ae.DataLoader(labels=labels)
        corpus, first = ld.corpus()
        assert corpus.dtype == np.int32 and corpus.shape == (sum(v.shape[0] for v in labels.values()), D)
        assert set(first) == set(labels) and first["train"] == 0
        at = 0
        for s in ("train", "val", "test"):  # the fixed order, whatever the dict's
            if s in labels:
                assert first[s] == at
                assert np.array_equal(corpus[at:at + labels[s].shape[0]], labels[s])
                at += labels[s].shape[0]
        assert ld.corpus()[0] is corpus  # built once
        for s in labels:
            rows, _ = ld.get_rows(s, 2)
            assert np.array_equal(corpus[rows], labels[s][:2])


class FakeCtx:
    def __init__(self, dims, device=0):
        self.dims, self.calls, self.corpus = dims, [], None

    def init_params(self, seed, lo, hi):
        pass

    def ae_corpus_load(self, tokens):
        self.corpus = np.array(tokens)

    def ae_step(self, tokens, dr, want_loss=True):
        self.calls.append(("ae_step", np.array(tokens), int(dr.step), want_loss))
        return 2.5 if want_loss else None

    def ae_step_rows(self, rows, dr, want_loss=True):
        self.calls.append(("ae_step_rows", self.corpus[rows], int(dr.step), want_loss))
        return 2.5 if want_loss else None

    def ae_evaluate(self, tokens, samples=False):
        self.calls.append(("ae_evaluate", np.array(tokens)))
        return 1.0, np.ones_like(tokens)

    def ae_evaluate_rows(self, rows, samples=False):
        self.calls.append(("ae_evaluate_rows", self.corpus[rows]))
        return 1.0, np.ones((len(rows), self.dims.T), np.int32)

    def adam_update(self, *a, stats=False):
        self.calls.append(("adam", stats))
        return (7.0, 3) if stats else None


@pytest.fixture()
def fake_ctx(pkg, monkeypatch):
    monkeypatch.setattr(pkg.binding, "Context", FakeCtx)
    return pkg


def test_trainer_routes_through_the_row_calls_after_load_corpus(fake_ctx):
    pkg = fake_ctx
    labels = {"train": split(10, 1), "val": split(6, 1) % 9 + 1}
    words = {str(i): f"w{i}" for i in range(1, 12)}
    runs = []
    for resident in (False, True):
        tr = pkg.ae.AETrainer(pkg.binding.Dims(3, 4, D, 11, 8, 8, 1, 0, 0, 0))
        loader = pkg.ae.DataLoader(labels=labels, ix_to_word=words)
        if resident:
            tr.load_corpus(loader)
            with pytest.raises(ValueError, match="another loader"):
                tr.train(pkg.ae.DataLoader(labels=labels), 1)
        else:
            with pytest.raises(ValueError, match="load_corpus"):
                tr.train_step_rows(np.arange(4))
        lines = []
        losses = tr.train(loader, 4, log=lines.append)  # the third batch wraps
        ev = tr.eval_split(loader, "val")
        runs.append((lines, losses, ev, tr.ctx.calls))
    (l0, s0, e0, c0), (l1, s1, e1, c1) = runs
    assert l0 == l1 and len(l0) == 4 and s0 == s1 and e0 == e1
    assert [c[0] for c in c0 if c[0] != "adam"] == ["ae_step"] * 4 + ["ae_evaluate"] * 2
    assert [c[0] for c in c1 if c[0] != "adam"] == ["ae_step_rows"] * 4 + ["ae_evaluate_rows"] * 2
    for a, b in zip(c0, c1):  # the same rows, dropout steps and flags, call for call
        assert len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))


def test_log_every_skips_the_loss_and_the_statistics(fake_ctx):
    pkg = fake_ctx
    tr = pkg.ae.AETrainer(pkg.binding.Dims(3, 4, D, 11, 8, 8, 1, 0, 0, 0))
    loader = pkg.ae.DataLoader(labels={"train": split(10, 1)})
    tr.load_corpus(loader)
    lines = []
    losses = tr.train(loader, 5, log=lines.append, log_every=2)
    assert [l.split(":")[0] for l in lines] == ["iter 2", "iter 4"] and losses == [2.5, 2.5]
    steps = [c for c in tr.ctx.calls if c[0] == "ae_step_rows"]
    assert [c[3] for c in steps] == [False, True, False, True, False]
    assert [c[1] for c in tr.ctx.calls if c[0] == "adam"] == [False, True, False, True, False]
    assert [c[2] for c in steps] == [1, 2, 3, 4, 5] and tr.iter == 6
