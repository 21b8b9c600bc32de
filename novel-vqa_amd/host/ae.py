"""Text auto-encoder pre-training (the reference's first stage, 001_train_autoencoder/001_train_arch1_text_autoencoder.lua
and 001_train_arch2_text_autoencoder.lua) on the library's NVQA_ARCH_AE1 / NVQA_ARCH_AE2 contexts: the data loader, the
training loop with its log line and learning-rate decay, eval_split, and the export that VQATrainer.init_from_autoencoder
reads (002_convert_text_model_arch1.lua:27-39; arch2: the table of lua/convert_ae_arch2.lua).
The weak-paired auto-encoder of the second stage (004_train_arch2_weakpaired_autoencoder_{vgg,inc}.lua) runs on an
NVQA_ARCH_AE2_WP context: WeakPairedDataLoader and WeakPairedAETrainer; its arch1 counterpart
(004_train_arch1_weakpaired_autoencoder_{vgg,inc}.lua, misc/AutoEncoder_vqa_arch.lua) on an NVQA_ARCH_AE1_WP context:
WeakPairedAE1Trainer.  Both take the features from the host, or -- with body=Vgg16 and a WeakPairedImageLoader -- run the
VGG-16 body on raw uint8 images inside the step, as the *_vgg scripts do (train_step_images)."""
import json

import numpy as np

from . import binding, h5, t7


class DataLoader:
    """misc/DataLoader.lua: sentences of `labels/<split>` ([N x D], 0 = null), iterated in order.
    `labels` may be given directly as {split: array} instead of an h5 file; ix_to_word comes from the json file.
    rank / world (data parallel): get_batch draws rank-disjoint sentences, see there."""

    def __init__(self, h5_file=None, json_file=None, labels=None, ix_to_word=None, rank=0, world=1):
        self.rank, self.world = int(rank), int(world)
        if not 0 <= self.rank < self.world:
            raise ValueError(f"rank {rank} outside 0..{world - 1}")
        if labels is None:
            with h5.File(h5_file) as f:
                labels = {s: np.asarray(f.read(f"labels/{s}")) for s in ("train", "val", "test") if self._has(f, s)}
        self.labels = {k: np.asarray(v).astype(np.int32) for k, v in labels.items()}
        if ix_to_word is None and json_file is not None:
            with open(json_file) as fh:
                ix_to_word = json.load(fh)["ix_to_word"]
        self.ix_to_word = ix_to_word or {}
        self.seq_length = next(iter(self.labels.values())).shape[1]
        self.iterators = {k: 1 for k in self.labels}
        self._corpus = None

    @staticmethod
    def _has(f, split):
        try:
            f.shape(f"labels/{split}")
            return True
        except Exception:
            return False

    def vocab_size(self):
        return len(self.ix_to_word)

    def reset_iterator(self, split):
        self.iterators[split] = 1

    def get_batch(self, split, batch_size, rank_stride=True):
        """getBatch (:58-89).  Returns (labels [batch_size x D], bounds dict(it_pos_now, it_max, wrapped)).
        On a wrap the rows up to the split's end are followed by the split's first rows and the iterator goes back to 1,
        so the next batch starts with those first rows again (the reference's behaviour, kept).
        world > 1: the iterator walks the split in strides of world * batch_size rows, as one process with that batch would,
        and this rank gets rows [rank * batch_size, (rank + 1) * batch_size) of each stride: the ranks' batches are disjoint,
        their union is the single-process batch, and every rank wraps in the same iteration.  rank_stride=False walks the split
        as a single process does, the same rows on every rank (AETrainer.eval_split)."""
        if self.world > 1 and rank_stride:
            rows, bounds = self._global_batch(split, batch_size * self.world)
            return rows[self.rank * batch_size:(self.rank + 1) * batch_size].copy(), bounds
        return self._global_batch(split, batch_size)

    def _global_batch(self, split, batch_size):
        rows, bounds = self._global_rows(split, batch_size)
        return self.labels[split][rows], bounds

    def _global_rows(self, split, batch_size):
        """the 0-based rows of the split that getBatch draws next (and the iterator's move)"""
        max_index = self.labels[split].shape[0]
        it = self.iterators[split]
        wrapped = False
        if it + batch_size - 1 > max_index:
            wrapped = True
            if it < max_index:
                num_left = max_index - it + 1
                rows = np.concatenate([np.arange(it - 1, max_index), np.arange(0, min(batch_size - num_left, max_index))])
            else:
                rows = np.arange(0, min(batch_size, max_index))
            self.iterators[split] = 1
        else:
            rows = np.arange(it - 1, it - 1 + batch_size)
            self.iterators[split] = it + batch_size
        return rows.astype(np.int64), {"it_pos_now": self.iterators[split], "it_max": max_index, "wrapped": wrapped}

    def corpus(self):
        """(tokens [N x D] int32, {split: first_row}): the splits one after the other -- train, val, test, then any other by
        name -- as one array for Context.ae_corpus_load; row i of a split is row first_row + i of it."""
        if self._corpus is None:
            order = [s for s in ("train", "val", "test") if s in self.labels] + sorted(set(self.labels) - {"train", "val", "test"})
            first, at = {}, 0
            for s in order:
                first[s] = at
                at += self.labels[s].shape[0]
            self._corpus = (np.ascontiguousarray(np.concatenate([self.labels[s] for s in order]), np.int32), first)
        return self._corpus

    def get_rows(self, split, batch_size, rank_stride=True):
        """get_batch by name: (rows int64 of corpus()[0], bounds), with corpus()[0][rows] equal to what get_batch returns for
        the same call.  Moves the same iterator in the same way (wrap, rank stride, back to 1 after a wrap)."""
        first = self.corpus()[1][split]
        if self.world > 1 and rank_stride:
            rows, bounds = self._global_rows(split, batch_size * self.world)
            rows = rows[self.rank * batch_size:(self.rank + 1) * batch_size]
        else:
            rows, bounds = self._global_rows(split, batch_size)
        return rows + first, bounds


def decode_sequence(ix_to_word, seq, end_token):
    """net_utils.decode_sequence: words up to the first END (or null) token, joined by spaces."""
    out = []
    for row in np.asarray(seq):
        words = []
        for ix in row:
            ix = int(ix)
            if ix == 0 or ix == end_token:
                break
            words.append(ix_to_word.get(str(ix), ix_to_word.get(ix, "UNK")))
        out.append(" ".join(words))
    return out


def _optim_update(ctx, optim, lr, lr0, alpha, beta, eps, wd, clamp, stats=True):
    """the scripts' `perform a parameter update` block: Context.optim_update of the named rule with the decayed rate lr --
    except sgd, which every script applies with the undecayed opt.learning_rate (lr0).  adam keeps its own entry point,
    nvqa_adam_update: the same kernel, state and bits as optim_update(OPT_ADAM)."""
    if optim == "adam":
        return ctx.adam_update(lr, alpha, beta, eps, wd, clamp, stats=stats)
    return ctx.optim_update(binding.OPT_RULES[optim], lr0 if optim == "sgd" else lr, alpha, beta, eps, wd, clamp, stats=stats)


# the training scripts' defaults that differ between the two auto-encoders (001_train_arch{1,2}_text_autoencoder.lua:32-50)
ARCH_DEFAULTS = {
    binding.ARCH_AE1: {"learning_rate": 1e-5, "max_iters": 75001, "save_model_every": 75000},
    binding.ARCH_AE2: {"learning_rate": 5e-5, "max_iters": 40001, "save_model_every": 40000},
}


class AETrainer:
    """The training script's loop on the library: ae_step (lossFun), the log line, the learning-rate decay and the
    update.  optim: the script's -optim, one of rmsprop | adagrad | sgd | sgdm | sgdmom | adam (misc/optim_updates.lua), each
    one fused pass of nvqa_optim_update's kernel with the log line's statistics reduced on the device.  sgd is applied with the
    undecayed learning_rate -- every reference script calls sgd(params, grad_params, opt.learning_rate) -- so it ignores
    learning_rate_decay_start; the other rules take the decayed rate.
    dims: binding.Dims with arch = ARCH_AE1 or ARCH_AE2, T = seq_length, I = C = A = 0 (the arch2 script forces 1 layer,
    :104; the library takes any L).  learning_rate None: the script's default.
    bf16: the step's bf16 operand mode (Context.ae_set_precision), for either arch.
    rank (data parallel, comm_init): the parameters come from `seed` on every rank (identical replicas), the dropout masks
    from seed + 1000 * rank, as in VQATrainer; dims.B is the batch per rank.  With a communicator the log line's loss,
    # updates and paramsNorm are the global values, so every rank prints the same line."""

    def __init__(self, dims, device=0, learning_rate=None, learning_rate_decay_start=-1, learning_rate_decay_every=50000,
                 optim="adam", optim_alpha=0.8, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=1e-6, grad_clip=0.1,
                 drop_prob=0.5, seed=123, bf16=False, rank=0):
        if dims.arch not in ARCH_DEFAULTS:
            raise ValueError("AETrainer needs dims.arch = ARCH_AE1 (3) or ARCH_AE2 (4)")
        if learning_rate is None:
            learning_rate = ARCH_DEFAULTS[dims.arch]["learning_rate"]
        if optim not in binding.OPT_RULES:
            raise ValueError("optim: rmsprop | adagrad | sgd | sgdm | sgdmom | adam (misc/optim_updates.lua)")
        self.dims = dims
        self.ctx = binding.Context(dims, device)
        self.learning_rate = learning_rate
        self.decay_start, self.decay_every = learning_rate_decay_start, learning_rate_decay_every
        self.optim = optim
        self.alpha, self.beta, self.eps = optim_alpha, optim_beta, optim_epsilon
        self.weight_decay, self.grad_clip = weight_decay, grad_clip
        self.drop_prob, self.seed = drop_prob, seed
        self.rank, self.world = int(rank), 1
        self.dropout_seed = seed + 1000 * self.rank  # ranks hold different sentences: identical masks would correlate them
        self.iter = 1
        self.bf16 = bool(bf16)
        self._resident = None  # the loader whose corpus is resident (load_corpus)
        self.ctx.init_params(seed, -0.08, 0.08)
        if self.bf16:  # bf16 operands for every dense product of the step and of eval_split (nvqa_ae_set_precision)
            self.ctx.ae_set_precision(1)

    def comm_init(self, rank, world, comm_id):
        """Join a data-parallel job (Context.ae_comm_init); rank must be the constructor's, which seeded the dropout masks."""
        if rank != self.rank:
            raise ValueError(f"comm_init(rank={rank}) on a trainer built with rank={self.rank}")
        self.ctx.ae_comm_init(rank, world, comm_id)
        self.world = int(world)

    def current_lr(self):
        """:342-347"""
        lr = self.learning_rate
        if self.decay_start >= 0 and self.iter > self.decay_start:
            lr *= 0.5 ** ((self.iter - self.decay_start) / self.decay_every)
        return lr

    def load_corpus(self, loader):
        """Make the loader's corpus resident in HBM (Context.ae_corpus_load of DataLoader.corpus()).  From here on train and
        eval_split name their batches by row ids (get_rows, ae_step_rows / ae_evaluate_rows): the same batches, the same bits."""
        self.ctx.ae_corpus_load(loader.corpus()[0])
        self._resident = loader

    def train_step(self, tokens, stats=True):
        """lossFun + log line + update of one iteration; returns (loss, # updates, paramsNorm, the log line).
        stats=False: the same step and update without the log line's figures (None in their place), so nothing is read back."""
        return self._step(lambda dr: self.ctx.ae_step(tokens, dr) if stats else self.ctx.ae_step(tokens, dr, want_loss=False), stats)

    def train_step_rows(self, rows, stats=True):
        """train_step on rows of the resident corpus (load_corpus); with stats=False the iteration only enqueues work."""
        if getattr(self, "_resident", None) is None:
            raise ValueError("train_step_rows before load_corpus")
        return self._step(lambda dr: self.ctx.ae_step_rows(rows, dr) if stats else self.ctx.ae_step_rows(rows, dr, want_loss=False), stats)

    def _step(self, step, stats):
        dr = binding.Dropout(1 if self.drop_prob > 0 else 0, self.drop_prob, self.dropout_seed, self.iter)
        loss = step(dr)
        norm = count = None
        out = _optim_update(self.ctx, self.optim, self.current_lr(), self.learning_rate, self.alpha, self.beta, self.eps,
                            self.weight_decay, self.grad_clip, stats)
        if stats:
            norm, count = out
        line = "iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f" % (self.iter, loss, count, norm) if stats else None
        self.iter += 1
        return loss, count, norm, line

    def _check_resident(self, loader):
        mine = getattr(self, "_resident", None)
        if mine is not None and loader is not mine:
            raise ValueError("the resident corpus is another loader's (load_corpus): its row ids mean nothing here")
        return mine is not None

    def train(self, loader, iters, log=print, log_every=1):
        """iters iterations.  log_every > 1: only the iterations whose number is a multiple of it are logged; the others run
        without the loss and the log line's statistics, so the host waits for nothing, and the returned losses are those of
        the logged iterations."""
        resident = self._check_resident(loader)
        losses = []
        for _ in range(iters):
            stats = self.iter % log_every == 0
            if resident:
                rows, _ = loader.get_rows("train", self.dims.B)
                loss, _, _, line = self.train_step_rows(rows, stats)
            else:
                batch, _ = loader.get_batch("train", self.dims.B)
                loss, _, _, line = self.train_step(batch, stats)
            if stats:
                losses.append(loss)
                if log:
                    log(line)
        return losses

    def sample(self, batch_or_rows, sample_max=1, temperature=1.0, beam_size=1, seed=0, logprobs=False, step=0, images=None):
        """sample(sents, opt) of misc/AutoEncoder_text_nostart.lua:134-210 under its option names: sample_max = 1 is the argmax,
        or -- with beam_size > 1 -- the beam search (:138); sample_max = 0 draws from exp(logprobs / temperature), keyed by
        (seed, step).  batch_or_rows: tokens [n x D], or a 1-d array of row ids of the resident corpus (load_corpus).  A beam
        needs beam_size decoder rows per sentence, so more than B // beam_size sentences are decoded in several calls (the
        multinomial draws are keyed by the row within a call: one call per B rows there).  Returns seq [n x D], or
        (seq, seqLogprobs) with logprobs=True."""
        x = np.asarray(batch_or_rows)
        beam = sample_max == 1 and beam_size > 1
        mode = binding.SAMPLE_BEAM if beam else (binding.SAMPLE_ARGMAX if sample_max == 1 else binding.SAMPLE_MULTINOMIAL)
        opts = binding.SampleOpts(mode, int(beam_size), float(temperature), 0, int(seed), int(step))
        per = max(1, self.dims.B // (int(beam_size) if beam else 1))
        out = []
        for i in range(0, x.shape[0], per):
            if x.ndim == 1:
                if getattr(self, "_resident", None) is None:
                    raise ValueError("sample(rows) before load_corpus")
                out.append(self.ctx.ae_sample_rows(x[i:i + per], opts, logprobs=True))
            else:
                img = None if images is None else np.asarray(images)[i:i + per]
                out.append(self.ctx.ae_sample(x[i:i + per], opts, images=img, logprobs=True))
        seq, lp = np.concatenate([o[0] for o in out]), np.concatenate([o[1] for o in out])
        return (seq, lp) if logprobs else seq

    def eval_split(self, loader, split="val", val_sentences_use=-1, sample_opts=None):
        """eval_split (:148-194): mean of the per-batch evaluate-mode losses, stopping when the split wraps or (when
        val_sentences_use > 0) once that many sentences were used; predictions are the greedy decodes through ix_to_word.
        sample_opts (a dict of sample()'s keywords; default None = the greedy path above, untouched): the predictions come from
        sample(batch, **sample_opts) instead, the loss as ever.
        (The arch1 reference's counter `n` is never incremented there, so only the wrap ends its loop.)
        ARCH_AE2 (001_train_arch2_text_autoencoder.lua:192-195): n grows by batch_size after every batch and the loop
        ends once n >= val_sentences_use, so a non-positive val_sentences_use evaluates one batch, as there.
        Data parallel: evaluation is rank-local (no collective) and walks the split without the rank stride, so with a
        DataLoader(rank=r, world=n) every rank evaluates the same rows and reports the same loss, as the Lua twins do."""
        resident = self._check_resident(loader)
        loader.reset_iterator(split)
        losses, preds, used, n = [], [], 0, 0
        end = self.dims.V + 1
        ae2 = self.dims.arch == binding.ARCH_AE2
        while True:
            if resident:
                rows, bounds = loader.get_rows(split, self.dims.B, rank_stride=False)
                batch = loader.corpus()[0][rows]
                loss, samples = self.ctx.ae_evaluate_rows(rows, samples=sample_opts is None)
            else:
                if getattr(loader, "world", 1) > 1:
                    batch, bounds = loader.get_batch(split, self.dims.B, rank_stride=False)
                else:
                    batch, bounds = loader.get_batch(split, self.dims.B)
                loss, samples = self.ctx.ae_evaluate(batch, samples=sample_opts is None)
            if sample_opts is not None:
                samples = self.sample(rows if resident else batch, **{**sample_opts, "logprobs": False})
            losses.append(loss)
            for p, a in zip(decode_sequence(loader.ix_to_word, samples, end), decode_sequence(loader.ix_to_word, batch, end)):
                used += 1
                preds.append({"seqNo": used, "prediction": p, "actual": a})
            n += self.dims.B
            if bounds["wrapped"]:
                break
            if ae2 and n >= val_sentences_use:
                break
            if not ae2 and val_sentences_use > 0 and used >= val_sentences_use:
                break
        return float(np.mean(losses)), preds

    def export_for_vqa(self, path):
        """002_convert_text_model_arch1.lua:27-39: {lookup = W_lk^T [E x (V+1)], encoder = the encoder segment} plus
        layout = 'nvqa' (the LSTM tensors are in include/nvqa_layout.h order), readable by init_from_autoencoder.
        ARCH_AE2: the table of lua/convert_ae_arch2.lua, {encoder, lookup_table = W_lk [(V+1) x E]}, plus the same mark;
        an arch2 VQATrainer reads it without encoder_perm."""
        d = self.dims
        x = self.ctx.get_params()
        seg = self.ctx.segments()
        w_lk = x[seg[0] + seg[1]:].reshape(d.V + 1, d.E)
        if d.arch == binding.ARCH_AE2:
            t7.save(path, {"encoder": x[:seg[0]].copy(), "lookup_table": np.ascontiguousarray(w_lk), "layout": t7.LAYOUT_MARK})
            return
        t7.save(path, {"lookup": np.ascontiguousarray(w_lk.T), "encoder": x[:seg[0]].copy(), "layout": t7.LAYOUT_MARK})

    def export_params(self, path):
        """The whole flat vector [encoder | decoder | lookup] (include/nvqa_layout.h order) as {params, layout = 'nvqa'}: what
        the weak-paired script's -start_from_text takes from a text checkpoint (protos.ae), read by
        WeakPairedAETrainer.init_from_text."""
        t7.save(path, {"params": self.ctx.get_params(), "layout": t7.LAYOUT_MARK})


class WeakPairedDataLoader(DataLoader):
    """misc/DataLoaderWeakPaired.lua: captions `labels/<split>` and their images walked in lockstep with DataLoader's wrap rule.
    The CNN body is frozen and runs outside the library, so the images come as its output: feats {split: [N x I]} (vgg:
    post-ReLU fc7, e.g. from nvqa_vgg16_fc7; inc: the pooled 2048-wide features), row i belonging to caption i."""

    def __init__(self, labels, feats, ix_to_word=None, json_file=None):
        super().__init__(labels=labels, ix_to_word=ix_to_word, json_file=json_file)
        self.feats = {k: np.asarray(v, np.float32) for k, v in feats.items()}
        for k, v in self.labels.items():
            if k in self.feats and self.feats[k].shape[0] != v.shape[0]:
                raise ValueError(f"split {k}: {v.shape[0]} captions but {self.feats[k].shape[0]} feature rows")

    def get_batch(self, split, batch_size):
        """getBatch (:58-103): (labels [batch_size x D], feats [batch_size x I], bounds), the rows of DataLoader.get_batch"""
        it, max_index = self.iterators[split], self.labels[split].shape[0]
        labels, bounds = super().get_batch(split, batch_size)
        if it + batch_size - 1 > max_index and it < max_index:
            num_left = max_index - it + 1
            rows = np.concatenate([np.arange(it - 1, max_index), np.arange(batch_size - num_left)])
        elif it + batch_size - 1 > max_index:
            rows = np.arange(batch_size)
        else:
            rows = np.arange(it - 1, it - 1 + batch_size)
        return labels, self.feats[split][rows], bounds


class WeakPairedImageLoader(DataLoader):
    """misc/DataLoaderWeakPaired.lua as the *_vgg scripts use it (:60-103): captions `labels/<split>` and the raw images
    `/images/<split>` ([N x 3 x S x S] uint8) walked linearly in lockstep, with DataLoader's wrap-around.
    images: {split: an array, or (h5 file path or h5.File, dataset name)}; a dataset is never read whole, only the rows of a
    batch (h5.File.read_rows, one call per run of consecutive rows: two on a wrap)."""

    def __init__(self, labels, images, ix_to_word=None, json_file=None):
        super().__init__(labels=labels, ix_to_word=ix_to_word, json_file=json_file)
        self.images, self._files = {}, []
        for k, v in images.items():
            if isinstance(v, tuple):
                f, name = v
                if isinstance(f, str):
                    f = h5.File(f)
                    self._files.append(f)
                shape, dt = f.shape(name), f.dtype(name)
                self.images[k] = (f, name)
            else:
                v = np.asarray(v)
                shape, dt = v.shape, v.dtype
                self.images[k] = v
            if dt != np.uint8 or len(shape) != 4 or shape[1] != 3 or shape[2] != shape[3]:
                raise ValueError(f"split {k}: images must be uint8 [N x 3 x S x S] (got {dt} {tuple(shape)})")
            if k in self.labels and self.labels[k].shape[0] != shape[0]:
                raise ValueError(f"split {k}: {self.labels[k].shape[0]} captions but {shape[0]} images")

    def close(self):
        for f in self._files:
            f.close()
        self._files = []

    def _image_rows(self, split, rows):
        src = self.images[split]
        if not isinstance(src, tuple):
            return np.ascontiguousarray(src[rows])
        f, name = src
        cuts = [0] + [i for i in range(1, len(rows)) if rows[i] != rows[i - 1] + 1] + [len(rows)]
        return np.concatenate([f.read_rows(name, int(rows[a]), int(rows[b - 1]) + 1) for a, b in zip(cuts[:-1], cuts[1:])])

    def get_batch(self, split, batch_size):
        """getBatch: (labels [batch_size x D], images [batch_size x 3 x S x S] uint8, bounds)"""
        rows, bounds = self._global_rows(split, batch_size)
        return self.labels[split][rows], self._image_rows(split, rows), bounds


# the VGG-16 body of the *_vgg scripts: drop6 / drop7 of the Caffe model (p = 0.5), the 224 window of net_utils.prepro
BODY_DROP_PROB = 0.5


def crop_origin_train(seed, it, S, hw):
    """The 0-based window origin (xoff, yoff) of training iteration `it`: net_utils.prepro's `torch.random(w - 224)` (1-based,
    uniform on 1..w-224) moved to 0-based, so uniform on 0..S-hw-1 -- the last valid origin S-hw is never drawn, as there.
    Drawn from a numpy generator seeded by (seed, it), behind the iteration's null-sentence / encoder-skip draw, so it depends
    on nothing before it.  S == hw: (0, 0)."""
    if S < hw:
        raise ValueError(f"source size {S} below the network's input {hw}")
    if S == hw:
        return 0, 0
    rng = np.random.default_rng([seed, it])
    rng.random()  # the iteration's null-sentence / skip draw
    xoff, yoff = rng.integers(0, S - hw, size=2)
    return int(xoff), int(yoff)


def crop_origin_eval(S, hw):
    """eval_split's central window: prepro's `math.ceil((w - 224) / 2)` (1-based) moved to 0-based; S == hw: (0, 0)."""
    if S < hw:
        raise ValueError(f"source size {S} below the network's input {hw}")
    o = max(0, -(-(S - hw) // 2) - 1)
    return o, o


def _is_raw_images(x):
    return getattr(x, "dtype", None) == np.uint8 and getattr(x, "ndim", 0) == 4


class _BodyInLoop:
    """What the two weak-paired trainers share once the body runs inside the step (body = binding.Vgg16)."""

    body = None
    body_dropout_in_eval = False

    def _need_body(self):
        if self.body is None:
            raise ValueError("raw images need the body in the loop: pass body=binding.Vgg16(...) to the trainer")
        if self.body.feature_dim != self.dims.I:
            raise ValueError(f"the body's feature width {self.body.feature_dim} is not dims.I = {self.dims.I}")
        return self.body

    def _body_train(self, images):
        """(xoff, yoff, body dropout) of the current training iteration: a random window, drop6 / drop7 live"""
        xoff, yoff = crop_origin_train(self.seed, self.iter, images.shape[-1], self._need_body().hw)
        return xoff, yoff, binding.Dropout(1, BODY_DROP_PROB, self.seed, self.iter)

    finetune_body = False
    _frozen_body_stats = None

    def _init_finetune_body(self, finetune_body):
        """finetune_body=True: once finetuning() holds, the step hands d(loss)/d(f^) to the body (the *_finetune step) and
        body.update runs the -cnn_optim rule on the whole body -- what the scripts do with protos.cnn from finetune_cnn_after on"""
        self.finetune_body = bool(finetune_body)
        if self.finetune_body:
            if self.body is None:
                raise ValueError("finetune_body=True needs body=binding.Vgg16(...)")
            self.body.train_enable(True)

    def _body_update(self, cnn_lr, scale):
        """the cnn update of the scripts on the body: wd through the scales, then the clamp, only when cnn_weight_decay > 0
        (arch2 :318-322), then -cnn_optim at the decayed rate.  Returns (cnnParamsNorm, # cnn updates) of the body."""
        clamp = self.grad_clip if self.cnn_weight_decay > 0 else 0.0
        self._frozen_body_stats = None
        return self.body.update(binding.CNN_OPT_RULES[self.cnn_optim], cnn_lr, self.cnn_alpha, self.cnn_beta, self.eps,
                                self.cnn_weight_decay, clamp, scale)

    def _body_stats_frozen(self):
        """the body's log figures before fine-tuning starts: its gradient is zero, so the count is that of the zero weights"""
        if self._frozen_body_stats is None:
            w = self.body.get_weights()
            self._frozen_body_stats = (float(np.sqrt((w.astype(np.float64) ** 2).sum())), int((w == 0).sum()))
        return self._frozen_body_stats

    def _body_eval(self, images):
        """(xoff, yoff, body dropout) of eval_split: the central window; the body in evaluate mode unless
        body_dropout_in_eval (the arch2 script never calls cnn:evaluate(), so its validation forwards drop too)"""
        xoff, yoff = crop_origin_eval(images.shape[-1], self._need_body().hw)
        dr = binding.Dropout(1, BODY_DROP_PROB, self.seed, self.iter) if self.body_dropout_in_eval else None
        return xoff, yoff, dr


# 004_train_arch2_weakpaired_autoencoder_{vgg,inc}.lua: the AE learning rate and the CNN feature width differ (:36-48, :62)
WEAKPAIRED_DEFAULTS = {"vgg": {"learning_rate": 1e-5, "I": 4096}, "inc": {"learning_rate": 3e-5, "I": 2048}}


class WeakPairedAETrainer(_BodyInLoop):
    """The weak-paired script's loop on an NVQA_ARCH_AE2_WP context: the null-sentence draw, ae_wp_step (lossFun), the log line
    with both update counts, the learning-rate decay, the -optim rule (default adam; AETrainer's six names, sgd undecayed as
    there) on [encoder | decoder] (the lookup table is frozen) and, once fine-tuning has started (finetune_cnn_after >= 0 and
    iter >= it), the -cnn_optim rule (sgd | sgdm | adam, default adam, all three at the decayed cnn rate) on the projection with
    its own state.
    dims: binding.Dims with arch = ARCH_AE2_WP, T = seq_length, I = the CNN feature width, C = A = 0.
    variant: 'vgg' or 'inc' (the default learning rate); learning_rate None: the variant's.

    The null-sentence draw replaces Lua's `math.random() <= rand_val` (:289-295), whose stream cannot be reproduced: a
    numpy generator seeded by (seed, iter), so the draw of an iteration does not depend on anything before it.

    body (binding.Vgg16 with feature width I): the frozen VGG-16 body runs inside the step on raw images -- train_step_images,
    and train / eval_split on a WeakPairedImageLoader.  Training cuts a random window per batch (crop_origin_train) and keeps
    drop6 / drop7 live (p = 0.5, the trainer's seed, the iteration as step); eval_split cuts the central window and runs the
    body in evaluate mode, the model as designed.  body_dropout_in_eval=True reproduces the script instead, which never calls
    cnn:evaluate() and so validates with both dropouts live.

    finetune_body=True (needs body): from finetune_cnn_after on the body learns too -- nvqa_ae_wp_step_images_finetune, then
    body.update with the -cnn_optim rule, the decayed cnn rate, cnn_weight_decay and the script's scale 0.01
    (cnnFinalLearningScales, :194).  The projection's update and the log line's cnn figures (the projection's, :353-354) are
    unchanged.  The default, False, keeps the projection-only meaning of finetune_cnn_after."""

    def __init__(self, dims, device=0, variant="vgg", learning_rate=None, learning_rate_decay_start=-1,
                 learning_rate_decay_every=50000, optim_alpha=0.8, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=1e-6,
                 grad_clip=0.1, drop_prob=0.5, rand_val=0.5, finetune_cnn_after=-1, cnn_optim_alpha=0.8, cnn_optim_beta=0.999,
                 cnn_learning_rate=1e-5, cnn_weight_decay=0.0, seed=123, bf16=False, optim="adam", cnn_optim="adam", body=None,
                 body_dropout_in_eval=False, finetune_body=False):
        self.body, self.body_dropout_in_eval = body, bool(body_dropout_in_eval)
        self._init_finetune_body(finetune_body)
        if optim not in binding.OPT_RULES:
            raise ValueError("optim: rmsprop | adagrad | sgd | sgdm | sgdmom | adam (misc/optim_updates.lua)")
        if cnn_optim not in binding.CNN_OPT_RULES:
            raise ValueError("cnn_optim: sgd | sgdm | adam")
        self.optim, self.cnn_optim = optim, cnn_optim
        if bf16:
            raise ValueError("bf16: the weak-paired auto-encoders have no bf16 operand mode (their step is launch-bound)")
        if dims.arch != binding.ARCH_AE2_WP:
            raise ValueError("WeakPairedAETrainer needs dims.arch = ARCH_AE2_WP (5)")
        if variant not in WEAKPAIRED_DEFAULTS:
            raise ValueError("variant: 'vgg' or 'inc'")
        self.dims = dims
        self.ctx = binding.Context(dims, device)
        self.learning_rate = WEAKPAIRED_DEFAULTS[variant]["learning_rate"] if learning_rate is None else learning_rate
        self.decay_start, self.decay_every = learning_rate_decay_start, learning_rate_decay_every
        self.alpha, self.beta, self.eps = optim_alpha, optim_beta, optim_epsilon
        self.weight_decay, self.grad_clip = weight_decay, grad_clip
        self.drop_prob, self.rand_val, self.seed = drop_prob, rand_val, seed
        self.finetune_cnn_after = finetune_cnn_after
        self.cnn_alpha, self.cnn_beta = cnn_optim_alpha, cnn_optim_beta
        self.cnn_learning_rate, self.cnn_weight_decay = cnn_learning_rate, cnn_weight_decay
        self.iter = 1
        self._frozen_cnn_stats = None
        self.ctx.init_params(seed, -0.08, 0.08)  # W_p uniform(-0.08, 0.08), b_p = 0 (build_cnn)

    def init_from_text(self, path):
        """-start_from_text: the text auto-encoder's [encoder | decoder | lookup], an AETrainer(ARCH_AE2).export_params table
        of the same dims (the flat vector is AE2's byte for byte)."""
        t = t7.load(path)
        if t.get("layout") != t7.LAYOUT_MARK:
            raise ValueError("text model table has no layout = 'nvqa' marker (AETrainer.export_params writes one)")
        self.set_params(t["params"])

    def set_params(self, x):
        x = np.asarray(x, np.float32).ravel()
        if x.size != self.ctx.param_count:
            raise ValueError(f"params has {x.size} values, the model wants {self.ctx.param_count}")
        self.ctx.set_params(x)

    def null_sentence(self, it=None):
        """True when iteration `it` feeds the null sentence to the encoder (probability rand_val)"""
        it = self.iter if it is None else it
        return bool(np.random.default_rng([self.seed, it]).random() <= self.rand_val)

    def current_lr(self):
        """(AE rate, cnn rate) after the decay (:443-451)"""
        f = 1.0
        if self.decay_start >= 0 and self.iter > self.decay_start:
            f = 0.5 ** ((self.iter - self.decay_start) / self.decay_every)
        return self.learning_rate * f, self.cnn_learning_rate * f

    def finetuning(self):
        return self.finetune_cnn_after >= 0 and self.iter >= self.finetune_cnn_after

    def _cnn_stats_frozen(self):
        """the log line's cnn figures while the projection is frozen: its gradient stays zero, so the count is that of the
        entries with |x| = 0 (computed once; the projection does not change)"""
        if self._frozen_cnn_stats is None:
            w, b = self.ctx.ae_wp_get_projection()
            self._frozen_cnn_stats = (float(np.sqrt((w.astype(np.float64) ** 2).sum())),
                                      int((w == 0).sum() + (b == 0).sum()))
        return self._frozen_cnn_stats

    def train_step_images(self, tokens, images_u8):
        """train_step with the body in the loop: images_u8 [B x 3 x S x S] uint8 instead of features"""
        return self.train_step(tokens, None, images_u8=images_u8)

    def train_step(self, tokens, feats, images_u8=None):
        """lossFun + log line + updates of one iteration; returns (loss, # updates, paramsNorm, # cnn updates, cnnParamsNorm,
        the log line)."""
        null = self.null_sentence()
        dr = binding.Dropout(1 if self.drop_prob > 0 else 0, self.drop_prob, self.seed, self.iter)
        if images_u8 is not None:
            xoff, yoff, bdr = self._body_train(images_u8)
            body_learns = self.finetune_body and self.finetuning()
            loss = self.ctx.ae_wp_step_images(self.body, images_u8, xoff, yoff, tokens, enc_tokens=None if null else tokens,
                                              body_dropout=bdr, dropout=dr, **({"finetune": True} if body_learns else {}))
        else:
            body_learns = False
            loss = self.ctx.ae_wp_step(feats, tokens, enc_tokens=None if null else tokens, dropout=dr)
        lr, cnn_lr = self.current_lr()
        if body_learns:
            self._body_update(cnn_lr, 0.01)
        norm, count = _optim_update(self.ctx, self.optim, lr, self.learning_rate, self.alpha, self.beta, self.eps,
                                    self.weight_decay, self.grad_clip)
        if self.finetuning():
            # wd then clamp, and only when cnn_weight_decay > 0, as the script's lossFun does (:318-322)
            clamp = self.grad_clip if self.cnn_weight_decay > 0 else 0.0
            if self.cnn_optim == "adam":  # its own entry point: the same kernel, state and bits as the rule OPT_ADAM
                cnn_norm, cnn_count = self.ctx.ae_wp_projection_adam(cnn_lr, self.cnn_alpha, self.cnn_beta, self.eps,
                                                                     self.cnn_weight_decay, clamp, stats=True)
            else:
                cnn_norm, cnn_count = self.ctx.ae_wp_projection_update(binding.CNN_OPT_RULES[self.cnn_optim], cnn_lr,
                                                                       self.cnn_alpha, self.cnn_beta, self.eps,
                                                                       self.cnn_weight_decay, clamp, stats=True)
            self._frozen_cnn_stats = None
        else:
            cnn_norm, cnn_count = self._cnn_stats_frozen()
        line = "iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f | # cnn updates: %4d | cnnParamsNorm: %.4f" % (
            self.iter, loss, count, norm, cnn_count, cnn_norm)
        self.iter += 1
        return loss, count, norm, cnn_count, cnn_norm, line

    def train(self, loader, iters, log=print):
        losses = []
        for _ in range(iters):
            labels, feats, _ = loader.get_batch("train", self.dims.B)
            out = self.train_step_images(labels, feats) if _is_raw_images(feats) else self.train_step(labels, feats)
            losses.append(out[0])
            if log:
                log(out[-1])
        return losses

    def eval_split(self, loader, split="val", val_sentences_use=-1):
        """eval_split (:199-260): AE2's stopping rule (n grows by batch_size; the loop ends on a wrap or once
        n >= val_sentences_use).  The loss and the greedy decodes take enc_tokens = tokens (forward{feats, labels, labels})."""
        loader.reset_iterator(split)
        losses, preds, used, n = [], [], 0, 0
        end = self.dims.V + 1
        while True:
            labels, feats, bounds = loader.get_batch(split, self.dims.B)
            if _is_raw_images(feats):  # a WeakPairedImageLoader: the body runs in front of the evaluation
                xoff, yoff, bdr = self._body_eval(feats)
                loss, samples = self.ctx.ae_wp_evaluate_images(self.body, feats, xoff, yoff, labels, enc_tokens=labels,
                                                               body_dropout=bdr, samples=True)
            else:
                loss, samples = self.ctx.ae_wp_evaluate(feats, labels, enc_tokens=labels, samples=True)
            losses.append(loss)
            for p, a in zip(decode_sequence(loader.ix_to_word, samples, end), decode_sequence(loader.ix_to_word, labels, end)):
                used += 1
                preds.append({"seqNo": used, "prediction": p, "actual": a})
            n += self.dims.B
            if bounds["wrapped"] or n >= val_sentences_use:
                break
        return float(np.mean(losses)), preds

    def export_for_vqa(self, path):
        """What 003_train_vqa_arch2/003_train_ae_based_wp_{vgg,inc}.lua take from the checkpoint (:76-77, 150-154, 174, 193):
        {encoder, lookup_table = W_lk [(V+1) x E], cnn_w = [W_p (E x I, row-major) | b_p], layout = 'nvqa'}; cnn_w is
        arch2's cnn segment as it stands, read by VQATrainer.init_from_autoencoder(..., with_cnn=True)."""
        d = self.dims
        x = self.ctx.get_params()
        seg = self.ctx.segments()
        w, b = self.ctx.ae_wp_get_projection()
        t7.save(path, {"encoder": x[:seg[0]].copy(), "lookup_table": np.ascontiguousarray(x[seg[0] + seg[1]:].reshape(d.V + 1, d.E)),
                       "cnn_w": np.concatenate([w.ravel(), b]), "layout": t7.LAYOUT_MARK})


# 004_train_arch1_weakpaired_autoencoder_{vgg,inc}.lua: batch size and CNN feature width differ (:43, :57); both use lr 3e-5
WEAKPAIRED1_DEFAULTS = {"vgg": {"batch_size": 16, "I": 4096}, "inc": {"batch_size": 10, "I": 2048}}


class WeakPairedAE1Trainer(_BodyInLoop):
    """The arch1 weak-paired script's loop on an NVQA_ARCH_AE1_WP context: the encoder-skip draw (:296-304), ae1_wp_step
    (lossFun), the log line, the learning-rate decay and the -optim rule (default adam; AETrainer's six names, sgd undecayed as
    there) over [encoder | decoder | multimodal] (clamp, then weight decay, :335-341).  The lookup table is frozen and lives outside the flat vector.
    dims: binding.Dims with arch = ARCH_AE1_WP, T = seq_length, L = 1, I = the CNN feature width, C = 2R, A = 0.

    The skip draw replaces Lua's `math.random() <= 0.5`, whose stream cannot be reproduced: a numpy generator seeded by
    (seed, iter), as WeakPairedAETrainer draws its null sentence.  The bridge (netdef.AxB's two Linear) starts from Torch's
    nn.Linear default, uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)), drawn here from the seed: the script clones a multimodal_net
    out of the text checkpoint (:150), a module the text model does not have.  The CNN body is frozen and runs outside the
    library, so the log line ends with paramsNorm (the script's two cnn figures describe that body).

    body (binding.Vgg16 with feature width I): the frozen body runs inside the step on raw images, as in WeakPairedAETrainer
    (train_step_images; train / eval_split on a WeakPairedImageLoader).  This script switches the body with cnn:training() /
    cnn:evaluate(), so eval_split's default -- no body dropout -- is also what the script does.

    finetune_body=True (needs body) with finetune_cnn_after / cnn_optim / cnn_optim_alpha / cnn_optim_beta / cnn_learning_rate /
    cnn_weight_decay, the script's options: from finetune_cnn_after on the step is nvqa_ae1_wp_step_images_finetune and
    body.update runs -cnn_optim at the decayed cnn rate with scale 1 (cnnFinalLearningScales is all ones, :182).  The log line
    then carries the script's two cnn fields, taken from the body (:374-375), and train_step returns them behind the line's
    other figures.  The default, False, keeps the trainer as it was: none of these options is read."""

    def __init__(self, dims, device=0, variant="vgg", learning_rate=3e-5, learning_rate_decay_start=-1,
                 learning_rate_decay_every=50000, optim_alpha=0.8, optim_beta=0.999, optim_epsilon=1e-8, weight_decay=1e-6,
                 grad_clip=0.1, drop_prob=0.5, skip_prob=0.5, seed=123, bf16=False, optim="adam", body=None,
                 body_dropout_in_eval=False, finetune_cnn_after=-1, cnn_optim="adam", cnn_optim_alpha=0.8, cnn_optim_beta=0.999,
                 cnn_learning_rate=1e-5, cnn_weight_decay=0.0, finetune_body=False):
        self.body, self.body_dropout_in_eval = body, bool(body_dropout_in_eval)
        self._init_finetune_body(finetune_body)
        if optim not in binding.OPT_RULES:
            raise ValueError("optim: rmsprop | adagrad | sgd | sgdm | sgdmom | adam (misc/optim_updates.lua)")
        if cnn_optim not in binding.CNN_OPT_RULES:
            raise ValueError("cnn_optim: sgd | sgdm | adam")
        self.optim, self.cnn_optim = optim, cnn_optim
        self.finetune_cnn_after = finetune_cnn_after
        self.cnn_alpha, self.cnn_beta = cnn_optim_alpha, cnn_optim_beta
        self.cnn_learning_rate, self.cnn_weight_decay = cnn_learning_rate, cnn_weight_decay
        if bf16:
            raise ValueError("bf16: the weak-paired auto-encoders have no bf16 operand mode (their step is launch-bound)")
        if dims.arch != binding.ARCH_AE1_WP:
            raise ValueError("WeakPairedAE1Trainer needs dims.arch = ARCH_AE1_WP (6)")
        if variant not in WEAKPAIRED1_DEFAULTS:
            raise ValueError("variant: 'vgg' or 'inc'")
        if dims.L != 1 or dims.C != 2 * dims.R:
            raise ValueError("ARCH_AE1_WP: L must be 1 and C must be 2R (AutoEncoder_vqa_arch.lua:24,33)")
        self.dims = dims
        self.variant = variant
        self.ctx = binding.Context(dims, device)
        self.learning_rate = learning_rate
        self.decay_start, self.decay_every = learning_rate_decay_start, learning_rate_decay_every
        self.alpha, self.beta, self.eps = optim_alpha, optim_beta, optim_epsilon
        self.weight_decay, self.grad_clip = weight_decay, grad_clip
        self.drop_prob, self.skip_prob, self.seed = drop_prob, skip_prob, seed
        self.mean_vector = None
        self.iter = 1
        self.ctx.init_params(seed, -0.08, 0.08)
        x = self.ctx.get_params()
        x[-self.ctx.segments()[2]:] = self.bridge_init(dims, seed)
        self.ctx.set_params(x)

    @staticmethod
    def default_dims(variant, T, V, E=512, R=512):
        """the scripts' dims: batch 16 / 10, I = 4096 / 2048, rnn_size = input_encoding_size = 512, one layer"""
        w = WEAKPAIRED1_DEFAULTS[variant]
        return binding.Dims(binding.ARCH_AE1_WP, w["batch_size"], T, V, E, R, 1, w["I"], 2 * R, 0)

    @staticmethod
    def bridge_init(dims, seed):
        """[W_q (2R x 2R) | b_q | W_v (2R x I) | b_v]: each Linear's weight and bias uniform(-1/sqrt(fan_in), 1/sqrt(fan_in))"""
        rng = np.random.default_rng([seed, 0x6272])
        n, out = 2 * dims.R, []
        for fan_in in (2 * dims.R, dims.I):
            k = 1.0 / np.sqrt(fan_in)
            out += [rng.uniform(-k, k, n * fan_in), rng.uniform(-k, k, n)]
        return np.concatenate(out).astype(np.float32)

    def init_from_text(self, path):
        """-start_from_text: encoder, decoder and lookup table of the arch1 text auto-encoder, an
        AETrainer(ARCH_AE1).export_params table [encoder | decoder | lookup] of the same B-independent dims.  The bridge keeps
        its initialisation."""
        t = t7.load(path)
        if t.get("layout") != t7.LAYOUT_MARK:
            raise ValueError("text model table has no layout = 'nvqa' marker (AETrainer.export_params writes one)")
        src = np.asarray(t["params"], np.float32).ravel()
        d, seg = self.dims, self.ctx.segments()
        n_lk = (d.V + 1) * d.E
        if src.size != seg[0] + seg[1] + n_lk:
            raise ValueError(f"text model has {src.size} values, the model wants {seg[0] + seg[1] + n_lk} = [encoder | decoder | lookup]")
        x = self.ctx.get_params()
        x[:seg[0] + seg[1]] = src[:seg[0] + seg[1]]
        self.ctx.set_params(x)
        self.ctx.ae1_wp_set_lookup(src[seg[0] + seg[1]:].reshape(d.V + 1, d.E))

    def set_mean_vector(self, v):
        """the corpus-mean sentence vector [2R] the skipped encoder is replaced by (-lstm_average_path's /mean_vector): an array,
        or the path of an HDF5 file holding /mean_vector"""
        if isinstance(v, str):
            with h5.File(v) as f:
                v = f.read("mean_vector")
        v = np.asarray(v, np.float32).ravel()
        if v.size != 2 * self.dims.R:
            raise ValueError(f"mean vector has {v.size} values, the model wants 2R = {2 * self.dims.R}")
        self.mean_vector = v
        return v

    def mean_sentence_vector(self, loader, split="train", max_sentences=-1):
        """The mean over a split's sentences of the evaluate-mode [c_T | h_T] (nvqa_ae1_wp_encode), accumulated in float64; the
        reference reads it from a file and ships no script that writes one.  Sets and returns it."""
        data = loader.labels[split]
        n = data.shape[0] if max_sentences <= 0 else min(max_sentences, data.shape[0])
        acc, used = np.zeros(2 * self.dims.R, np.float64), 0
        for i in range(0, n, self.dims.B):
            rows = data[i:min(i + self.dims.B, n)]
            rows = rows[(rows != 0).any(axis=1)]
            if rows.shape[0] == 0:
                continue
            acc += self.ctx.ae1_wp_encode(rows).astype(np.float64).sum(axis=0)
            used += rows.shape[0]
        if used == 0:
            raise ValueError("no sentence to encode")
        return self.set_mean_vector(acc / used)

    def skip_encoder(self, it=None):
        """True when iteration `it` skips the encoder (probability skip_prob)"""
        it = self.iter if it is None else it
        return bool(np.random.default_rng([self.seed, it]).random() <= self.skip_prob)

    def current_lr(self):
        lr = self.learning_rate
        if self.decay_start >= 0 and self.iter > self.decay_start:
            lr *= 0.5 ** ((self.iter - self.decay_start) / self.decay_every)
        return lr

    def finetuning(self):
        return self.finetune_cnn_after >= 0 and self.iter >= self.finetune_cnn_after

    def train_step_images(self, tokens, images_u8):
        """train_step with the body in the loop: images_u8 [B x 3 x S x S] uint8 instead of features"""
        return self.train_step(tokens, None, images_u8=images_u8)

    def train_step(self, tokens, feats, images_u8=None):
        """lossFun + log line + update of one iteration; returns (loss, # updates, paramsNorm, skipped, the log line); with
        finetune_body (loss, # updates, paramsNorm, skipped, # cnn updates, cnnParamsNorm, the log line)."""
        skip = self.skip_encoder()
        if skip and self.mean_vector is None:
            raise ValueError("the encoder is skipped in this iteration: set_mean_vector / mean_sentence_vector first")
        dr = binding.Dropout(1 if self.drop_prob > 0 else 0, self.drop_prob, self.seed, self.iter)
        enc = {"enc_state": np.tile(self.mean_vector, (self.dims.B, 1))} if skip else {"enc_tokens": tokens}
        if images_u8 is not None:
            xoff, yoff, bdr = self._body_train(images_u8)
            body_learns = self.finetune_body and self.finetuning()
            loss = self.ctx.ae1_wp_step_images(self.body, images_u8, xoff, yoff, tokens, body_dropout=bdr, dropout=dr,
                                               **({"finetune": True} if body_learns else {}), **enc)
        else:
            body_learns = False
            loss = self.ctx.ae1_wp_step(feats, tokens, dropout=dr, **enc)
        lr = self.current_lr()
        norm, count = _optim_update(self.ctx, self.optim, lr, self.learning_rate, self.alpha, self.beta, self.eps,
                                    self.weight_decay, self.grad_clip)
        line = "iter %d: loss: %.3f | # updates: %4d | paramsNorm: %.4f" % (self.iter, loss, count, norm)
        if not self.finetune_body:
            self.iter += 1
            return loss, count, norm, skip, line
        # the cnn rate decays with the AE rate (:465-473)
        cnn_norm, cnn_count = (self._body_update(self.cnn_learning_rate * lr / self.learning_rate, 1.0) if body_learns
                               else self._body_stats_frozen())
        line += " | # cnn updates: %4d | cnnParamsNorm: %.4f" % (cnn_count, cnn_norm)
        self.iter += 1
        return loss, count, norm, skip, cnn_count, cnn_norm, line

    def train(self, loader, iters, log=print):
        losses = []
        for _ in range(iters):
            labels, feats, _ = loader.get_batch("train", self.dims.B)
            out = self.train_step_images(labels, feats) if _is_raw_images(feats) else self.train_step(labels, feats)
            losses.append(out[0])
            if log:
                log(out[-1])
        return losses

    def eval_split(self, loader, split="val", val_sentences_use=-1):
        """eval_split (:212-275): forward{feats, labels, labels, 0} -- the encoder runs on the captions -- with the arch2
        scripts' stopping rule (n grows by batch_size; a wrap or n >= val_sentences_use ends the loop)."""
        loader.reset_iterator(split)
        losses, preds, used, n = [], [], 0, 0
        end = self.dims.V + 1
        while True:
            labels, feats, bounds = loader.get_batch(split, self.dims.B)
            if _is_raw_images(feats):  # a WeakPairedImageLoader: the body runs in front of the evaluation
                xoff, yoff, bdr = self._body_eval(feats)
                loss, samples = self.ctx.ae1_wp_evaluate_images(self.body, feats, xoff, yoff, labels, enc_tokens=labels,
                                                                body_dropout=bdr, samples=True)
            else:
                loss, samples = self.ctx.ae1_wp_evaluate(feats, labels, enc_tokens=labels, samples=True)
            losses.append(loss)
            for p, a in zip(decode_sequence(loader.ix_to_word, samples, end), decode_sequence(loader.ix_to_word, labels, end)):
                used += 1
                preds.append({"seqNo": used, "prediction": p, "actual": a})
            n += self.dims.B
            if bounds["wrapped"] or n >= val_sentences_use:
                break
        return float(np.mean(losses)), preds

    def export_for_vqa(self, path):
        """005_convert_weakpaired_model_arch1.lua: {lookup = W_lk^T [E x (V+1)], encoder = the encoder's flat parameters,
        multimodal = [W_q | b_q | W_v | b_v] flat}, plus layout = 'nvqa': what
        VQATrainer.init_from_autoencoder(..., with_multimodal=True) reads on an arch1 trainer with set_fusion(1)."""
        x = self.ctx.get_params()
        seg = self.ctx.segments()
        t7.save(path, {"lookup": np.ascontiguousarray(self.ctx.ae1_wp_get_lookup().T), "encoder": x[:seg[0]].copy(),
                       "multimodal": x[seg[0] + seg[1]:].copy(), "layout": t7.LAYOUT_MARK})
