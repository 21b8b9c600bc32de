#!/usr/bin/env python3
"""ae_bench.py -- the text auto-encoder's training step (nvqa_ae_step + nvqa_adam_update) at the reference's default
shape (001_train_arch1_text_autoencoder.lua: B = 1000, seq_length D = 16, E = R = 512, 1 layer, dropout 0.5, Adam) with
the VQA vocabulary (V = 14773), on random sentences of lengths U{3..16}.  Prints ONE JSON line: ms per step and
sentences/s (median over timed blocks after warm-up), the per-group profile of a separate profiled pass, and the
step's fraction of the f32 MFMA roofline (FLOPs computed from the shape, 3 x forward).
--arch 2: the image-first-token auto-encoder (001_train_arch2_text_autoencoder.lua, NVQA_ARCH_AE2) at the same shape,
with the text script's zero image rows (nvqa_ae_step on an AE2 context) and its learning rate 5e-5.
--arch 5: the weak-paired auto-encoder (004_train_arch2_weakpaired_autoencoder_vgg.lua, NVQA_ARCH_AE2_WP): nvqa_ae_wp_step on
random post-ReLU-like features [B x I] (--I, default 4096), the encoder fed the null sentence in a share --null-share of the
steps (a fixed draw per step) and the captions otherwise, then nvqa_adam_update on [encoder | decoder] (the script's default
-finetune_cnn_after -1 never updates the projection).  The reference shape is --B 20 --null-share 0.5.
--arch 6: the arch1 weak-paired auto-encoder (004_train_arch1_weakpaired_autoencoder_vgg.lua, NVQA_ARCH_AE1_WP):
nvqa_ae1_wp_step on the same features, the encoder skipped (enc_state = one vector repeated over the batch) in a share
--null-share of the steps and run on the captions otherwise, then nvqa_adam_update on [encoder | decoder | multimodal].  The
reference shape is --B 16 --null-share 0.5 (inc: --B 10 --I 2048).
--bf16 (--arch 1 | 2): the step's bf16 operand mode (nvqa_ae_set_precision); the line then carries "bf16": 1 and the step's
fraction of the bf16 MFMA roofline as well.
--world N (--arch 1 | 2): data parallel (nvqa_ae_comm_init) as ONE process, rank 0 of N, on whatever collective library
NVQA_RCCL_LIB names -- on a one-GPU machine the stand-in tests/shim/libnccl_shim.so, whose all-reduce returns N x send
(NCCL_SHIM_CUS = n gives it the footprint and the duration of a collective over 150 GB/s links); any other library is
refused, since a real one would wait for the N - 1 ranks this tool never starts.  A second context of the same
shape without a communicator is timed in the same job, the two alternating block by block; the line carries both
("ms_per_step" without, "ms_per_step_world" with the communicator), their difference and the communicator context's profile.
--optim RULE: the update of every step is nvqa_optim_update of that rule of misc/optim_updates.lua (rmsprop | adagrad | sgd |
sgdm | sgdmom | adam) with the scripts' alpha 0.8 / beta 0.999; the line then carries "optim".  The default, adam, runs
nvqa_adam_update as ever.
--resident (--arch 1 | 2, no --world): the same batches as one corpus in HBM (nvqa_ae_corpus_load), every step named by its row
ids (nvqa_ae_step_rows); the line then carries "resident": 1.  Without the flag the tool runs as ever.
--images (--arch 5 | 6): the weak-paired step with the VGG-16 body in the loop at the reference's shape -- B = 20 (arch 5) / 16
(arch 6) unless --B is given, uint8 images of --S 256, the full-width body on 224 windows with drop6 / drop7 live and synthetic
He-scaled weights -- in two arms that alternate block by block in this one job: "in_loop" = nvqa_ae*_wp_step_images (the
features stay on the device), "composed" = nvqa_vgg16_fc7_raw to the host and the host-fed step on what came back.  Both arms
compute the same bits per step and end every step with nvqa_adam_update; a block is timed around a final synchronise.  The
line carries both arms' ms per step (median over blocks), their block times and spreads and the ratio.

--finetune (--arch 5 | 6): the same shape with the body fine-tuning, in two arms that alternate block by
block: "frozen" = nvqa_ae*_wp_step_images + nvqa_adam_update, "finetune" = nvqa_ae*_wp_step_images_finetune + nvqa_adam_update
+ nvqa_vgg16_update (adam, scale 0.01 for arch 5 and 1 for arch 6) on a training-enabled extractor of their own each.  A block
ends with both streams drained (the last update of a block returns its statistics).  The line carries both arms' ms per step,
block times and spreads, and finetune_over_frozen.

    python novel-vqa_amd/tools/ae_bench.py [--arch 1|2|5|6] [--bf16] [--I 4096 --null-share 0.5] [--world N] [--resident] [--optim RULE]
                                           [--images | --finetune [--S 256 --body-div 1 --body-hw 224]]
                                           [--blocks 5 --steps 10 --warmup 5] [--out FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import __graft_entry__ as ge  # noqa: E402

FP32_MFMA_PEAK_TFLOPS = 157.3  # MI355X_MICROARCH.md "Peak FP32 (matrix)"
BF16_MFMA_PEAK_TFLOPS = 16 * FP32_MFMA_PEAK_TFLOPS  # the same row: the f32 rate is 1/16 of the BF16 MFMA rate (~2.5 PF dense)


def step_flops(B, T, V, E, R, L, arch=1, te=None, I=0):
    """3 x forward of a batch whose tmax is T: T (arch 2: T + 2) encoder + T+1 decoder LSTM steps, T+1 projections.
    arch 5: te encoder steps (2 + the encoder tokens' tmax), T+1 decoder steps, and the feature projection (forward and
    dW_p: 2 x 2 B E I; no d(features))"""
    lstm = sum(2 * B * 4 * R * ((E if l == 0 else R) + R) for l in range(L))
    if arch == 5:
        return 3 * ((te + T + 1) * lstm + (T + 1) * 2.0 * B * R * (V + 1)) + 4.0 * B * E * I
    if arch == 6:  # te encoder steps (0: skipped); the bridge: forward and weight gradients of both Linear, dj when the encoder ran
        bridge = 4.0 * B * 2 * R * (2 * R + I) + (2.0 * B * 2 * R * 2 * R if te else 0.0)
        return 3 * ((te + T + 1) * lstm + (T + 1) * 2.0 * B * R * (V + 1)) + bridge
    fwd = (2 * T + 1 + (2 if arch == 2 else 0)) * lstm + (T + 1) * 2.0 * B * R * (V + 1)
    return 3 * fwd


def body_weights(vgg_div, hw, count, seed=7):
    """He-scaled random weights in nvqa_vgg16_set_weights order (no caffemodel here): activations keep their scale layer by layer"""
    rng = np.random.default_rng(seed)
    parts, cin = [], 3
    for c in (64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512):
        co = max(1, c // vgg_div)
        parts += [rng.standard_normal(co * cin * 9, np.float32) * np.float32(np.sqrt(2.0 / (cin * 9))), rng.uniform(0.0, 0.1, co).astype(np.float32)]
        cin = co
    F = max(4, 4096 // vgg_div)
    for k in (cin * (hw // 32) ** 2, F):
        parts += [rng.standard_normal(F * k, np.float32) * np.float32(np.sqrt(2.0 / k)), rng.uniform(0.0, 0.1, F).astype(np.float32)]
    w = np.concatenate(parts)
    assert w.size == count
    return w


def images_main(a, pkg):
    """--images: the in-loop step against the composed route, alternating in one job"""
    b = pkg.binding
    B = a.B if a.B != 1000 else {5: 20, 6: 16}[a.arch]
    vgg = b.Vgg16(0, a.body_div, a.body_hw, max_batch=B)
    vgg.set_weights(body_weights(a.body_div, a.body_hw, vgg.weight_count))
    I = vgg.feature_dim
    arch = {5: b.ARCH_AE2_WP, 6: b.ARCH_AE1_WP}[a.arch]
    dims = b.Dims(arch, B, a.D, a.V, a.E, a.R, a.L, I, 2 * a.R if a.arch == 6 else 0, 0)
    lr = {5: 1e-5, 6: 3e-5}[a.arch]
    enc_state = np.tile(np.random.default_rng(3).uniform(-0.5, 0.5, 2 * a.R).astype(np.float32), (B, 1))

    def make_ctx():  # one context per arm, the same start
        ctx = b.Context(dims, 0)
        ctx.init_params(123, -0.08, 0.08)
        if a.arch == 6:
            x = ctx.get_params()
            x[-ctx.segments()[2]:] = pkg.ae.WeakPairedAE1Trainer.bridge_init(dims, 123)
            ctx.set_params(x)
            ctx.ae1_wp_set_lookup(np.random.default_rng(2).uniform(-0.08, 0.08, (a.V + 1, a.E)).astype(np.float32))
        return ctx

    rng = np.random.default_rng(0)
    batches, images = [], []
    for _ in range(4):
        lens = rng.integers(3, a.D + 1, B)
        tok = np.zeros((B, a.D), np.int32)
        for i, n in enumerate(lens):
            tok[i, :n] = rng.integers(1, a.V + 1, n)
        batches.append(tok)
        images.append(rng.integers(0, 256, (B, 3, a.S, a.S), dtype=np.uint8))
    null = np.random.default_rng(1).random(4096) < a.null_share
    arms = {"frozen": make_ctx(), "finetune": make_ctx()} if a.finetune else {"in_loop": make_ctx(), "composed": make_ctx()}
    its = {k: 0 for k in arms}
    if a.finetune:  # the fine-tuning arm moves its body: one extractor per arm
        tuned = b.Vgg16(0, a.body_div, a.body_hw, max_batch=B)
        tuned.set_weights(vgg.get_weights())
        tuned.train_enable(True)

    def one_step(arm, want_loss=False, last=False):
        its[arm] += 1
        it = its[arm]
        ctx, k = arms[arm], it % len(batches)
        xoff, yoff = pkg.ae.crop_origin_train(123, it, a.S, a.body_hw)
        bdr, dr = b.Dropout(1, 0.5, 123, it), b.Dropout(1, 0.5, 123, it)
        skip = bool(null[it % null.size])
        if a.arch == 5:
            enc = {"enc_tokens": None if skip else batches[k]}
        else:
            enc = {"enc_state": enc_state} if skip else {"enc_tokens": batches[k]}
        if arm in ("in_loop", "frozen"):
            step = ctx.ae_wp_step_images if a.arch == 5 else ctx.ae1_wp_step_images
            loss = step(vgg, images[k], xoff, yoff, batches[k], body_dropout=bdr, dropout=dr, want_loss=want_loss, **enc)
        elif arm == "finetune":
            step = ctx.ae_wp_step_images if a.arch == 5 else ctx.ae1_wp_step_images
            loss = step(tuned, images[k], xoff, yoff, batches[k], body_dropout=bdr, dropout=dr, want_loss=want_loss, finetune=True, **enc)
            ctx.adam_update(lr, 0.8, 0.999, 1e-8, 1e-6, 0.1)
            tuned.update(b.OPT_ADAM, 1e-5, 0.8, 0.999, 1e-8, 0.0, 0.0, 0.01 if a.arch == 5 else 1.0, want_stats=last)  # last: drains the body's stream
            return loss
        else:
            feats = vgg.fc7_raw(images[k], xoff, yoff, dropout=bdr)  # to the host and back
            step = ctx.ae_wp_step if a.arch == 5 else ctx.ae1_wp_step
            loss = step(feats, batches[k], dropout=dr, want_loss=want_loss, **enc)
        ctx.adam_update(lr, 0.8, 0.999, 1e-8, 1e-6, 0.1)
        return loss

    def timed_block(arm):
        t0 = time.perf_counter()
        for i in range(a.steps):
            one_step(arm, last=i == a.steps - 1)
        arms[arm].sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for arm in arms:
        for _ in range(a.warmup):
            one_step(arm)
        arms[arm].sync()
    blocks = {k: [] for k in arms}
    for _ in range(a.blocks):
        for arm in arms:
            blocks[arm].append(timed_block(arm))
    # both arms have run the same steps: the next one must give the same loss, bit for bit (--finetune: the bodies differ by now)
    losses = {arm: one_step(arm, want_loss=True, last=True) for arm in arms}
    for c in arms.values():
        c.close()
    vgg.close()
    med = {k: float(np.median(v)) for k, v in blocks.items()}
    if a.finetune:
        tuned.close()
        line = {"workload": "ae_arch%d_weakpaired_finetune" % a.arch, "B": B, "S": a.S, "body_div": a.body_div, "body_hw": a.body_hw,
                "I": I, "D": a.D, "V": a.V, "E": a.E, "R": a.R, "L": a.L, "null_share": a.null_share, "blocks": a.blocks,
                "steps_per_block": a.steps, "warmup": a.warmup, "order": list(arms), "loss_frozen": losses["frozen"],
                "loss_finetune": losses["finetune"]}
        for k in arms:
            line["ms_per_step_" + k] = round(med[k], 4)
            line["block_ms_" + k] = [round(x, 4) for x in blocks[k]]
            line["block_spread_pct_" + k] = round(100.0 * (max(blocks[k]) - min(blocks[k])) / med[k], 2)
        line["finetune_over_frozen"] = round(med["finetune"] / med["frozen"], 4)
        s = json.dumps(line)
        print(s)
        if a.out:
            with open(a.out, "w") as f:
                f.write(s + "\n")
        return
    line = {"workload": "ae_arch%d_weakpaired_images" % a.arch, "B": B, "S": a.S, "body_div": a.body_div, "body_hw": a.body_hw,
            "I": I, "D": a.D, "V": a.V, "E": a.E, "R": a.R, "L": a.L, "null_share": a.null_share,
            "blocks": a.blocks, "steps_per_block": a.steps, "warmup": a.warmup, "order": list(arms),
            "loss_in_loop": losses["in_loop"], "loss_composed": losses["composed"],
            "losses_bit_equal": bool(losses["in_loop"] == losses["composed"])}
    for k in arms:
        line["ms_per_step_" + k] = round(med[k], 4)
        line["block_ms_" + k] = [round(x, 4) for x in blocks[k]]
        line["block_spread_pct_" + k] = round(100.0 * (max(blocks[k]) - min(blocks[k])) / med[k], 2)
    line["composed_over_in_loop"] = round(med["composed"] / med["in_loop"], 4)
    line["images_per_s_in_loop"] = round(B / (med["in_loop"] * 1e-3), 1)
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--arch", type=int, default=1, choices=(1, 2, 5, 6))
    ap.add_argument("--B", type=int, default=1000)
    ap.add_argument("--D", type=int, default=16)
    ap.add_argument("--V", type=int, default=14773)
    ap.add_argument("--E", type=int, default=512)
    ap.add_argument("--R", type=int, default=512)
    ap.add_argument("--L", type=int, default=1)
    ap.add_argument("--I", type=int, default=4096)
    ap.add_argument("--null-share", type=float, default=0.5)
    ap.add_argument("--blocks", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--bf16", action="store_true")
    ap.add_argument("--world", type=int, default=1)
    ap.add_argument("--resident", action="store_true")
    ap.add_argument("--optim", default="adam", choices=("rmsprop", "adagrad", "sgd", "sgdm", "sgdmom", "adam"))
    ap.add_argument("--images", action="store_true")
    ap.add_argument("--finetune", action="store_true")
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--body-div", type=int, default=1)
    ap.add_argument("--body-hw", type=int, default=224)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if a.images or a.finetune:
        if a.arch not in (5, 6) or a.world > 1 or a.resident or a.bf16 or a.optim != "adam":
            ap.error("--images: the body in the loop is for --arch 5 | 6 alone")
        return images_main(a, ge.load_package())
    if a.world < 1 or (a.world > 1 and a.arch not in (1, 2)):
        ap.error("--world: data parallel is for --arch 1 | 2 (the weak-paired contexts refuse a communicator)")
    if a.resident and (a.arch not in (1, 2) or a.world > 1):
        ap.error("--resident: the resident corpus is for --arch 1 | 2, timed without --world")
    if a.bf16 and a.arch not in (1, 2):
        ap.error("--bf16: the weak-paired auto-encoders have no bf16 operand mode")
    pkg = ge.load_package()
    b = pkg.binding
    arch = {1: b.ARCH_AE1, 2: b.ARCH_AE2, 5: b.ARCH_AE2_WP, 6: b.ARCH_AE1_WP}[a.arch]
    I = a.I if a.arch in (5, 6) else 0
    dims = b.Dims(arch, a.B, a.D, a.V, a.E, a.R, a.L, I, 2 * a.R if a.arch == 6 else 0, 0)
    lr = {1: 1e-5, 2: 5e-5, 5: 1e-5, 6: 3e-5}[a.arch]
    ctx = b.Context(dims, 0)
    ctx.init_params(123, -0.08, 0.08)
    if a.bf16:
        ctx.ae_set_precision(1)
    enc_state = None
    if a.arch == 6:  # the bridge and the frozen lookup as WeakPairedAE1Trainer sets them up
        x = ctx.get_params()
        x[-ctx.segments()[2]:] = pkg.ae.WeakPairedAE1Trainer.bridge_init(dims, 123)
        ctx.set_params(x)
        ctx.ae1_wp_set_lookup(np.random.default_rng(2).uniform(-0.08, 0.08, (a.V + 1, a.E)).astype(np.float32))
        enc_state = np.tile(np.random.default_rng(3).uniform(-0.5, 0.5, 2 * a.R).astype(np.float32), (a.B, 1))
    ctxw = None
    if a.world > 1:  # the same shape and parameters with a communicator: rank 0 of --world
        ctxw = b.Context(dims, 0)
        # one process is one rank: a real collective library would wait in ncclCommInitRank for world - 1 ranks that never come
        import ctypes
        lib_path = ctxw.comm_library()
        if not hasattr(ctypes.CDLL(lib_path), "nccl_shim_calls"):
            ctxw.close()
            ctx.close()
            sys.exit(f"--world {a.world}: {lib_path} is not the one-process stand-in (tests/shim/libnccl_shim.so); set "
                     "NVQA_RCCL_LIB to it -- with a real collective library this single rank would hang waiting for the others")
        ctxw.init_params(123, -0.08, 0.08)
        if a.bf16:
            ctxw.ae_set_precision(1)
        ctxw.ae_comm_init(0, a.world, ctxw.comm_unique_id())
    rng = np.random.default_rng(0)
    batches = []
    for _ in range(8):
        lens = rng.integers(3, a.D + 1, a.B)
        tok = np.zeros((a.B, a.D), np.int32)
        for i, n in enumerate(lens):
            tok[i, :n] = rng.integers(1, a.V + 1, n)
        batches.append(tok)
    rows = []
    if a.resident:  # batch k = rows [k B, (k + 1) B) of the corpus
        ctx.ae_corpus_load(np.concatenate(batches))
        rows = [np.arange(k * a.B, (k + 1) * a.B, dtype=np.int64) for k in range(len(batches))]
    feats = []
    if a.arch in (5, 6):
        for _ in batches:
            f = rng.uniform(0, 1, (a.B, I)).astype(np.float32)
            f[rng.uniform(0, 1, (a.B, I)) < 0.5] = 0.0
            feats.append(f)
    # the null-sentence draw of step k (a fixed sequence, so that every run times the same mix)
    null = np.random.default_rng(1).random(4096) < a.null_share
    it = [0]

    def one_step(ctx=ctx):
        it[0] += 1
        k = it[0] % len(batches)
        dr = b.Dropout(1, 0.5, 123, it[0])
        if a.arch == 5:
            ctx.ae_wp_step(feats[k], batches[k], enc_tokens=None if null[it[0] % null.size] else batches[k], dropout=dr,
                           want_loss=False)
        elif a.arch == 6:
            if null[it[0] % null.size]:
                ctx.ae1_wp_step(feats[k], batches[k], enc_state=enc_state, dropout=dr, want_loss=False)
            else:
                ctx.ae1_wp_step(feats[k], batches[k], enc_tokens=batches[k], dropout=dr, want_loss=False)
        elif a.resident:
            ctx.ae_step_rows(rows[k], dr, want_loss=False)
        else:
            ctx.ae_step(batches[k], dr, want_loss=False)
        if a.optim == "adam":
            ctx.adam_update(lr, 0.8, 0.999, 1e-8, 1e-6, 0.1)
        else:
            ctx.optim_update(b.OPT_RULES[a.optim], lr, 0.8, 0.999, 1e-8, 1e-6, 0.1)

    def timed_block(c):
        t0 = time.perf_counter()
        for _ in range(a.steps):
            one_step(c)
        c.sync()
        return (time.perf_counter() - t0) * 1e3 / a.steps

    for c in (ctx, ctxw) if ctxw else (ctx,):
        for _ in range(a.warmup):
            one_step(c)
        c.sync()
    block_ms, block_ms_world = [], []
    for _ in range(a.blocks):  # (--world: the two contexts alternate, so that drift hits both alike)
        block_ms.append(timed_block(ctx))
        if ctxw:
            block_ms_world.append(timed_block(ctxw))
    ms = float(np.median(block_ms))
    timed = range(a.warmup + 1, a.warmup + a.blocks * a.steps + 1)  # the iteration numbers of the timed steps
    if a.arch == 5:
        loss = ctx.ae_wp_step(feats[0], batches[0], enc_tokens=batches[0], dropout=b.Dropout(1, 0.5, 123, 0))
    elif a.arch == 6:
        loss = ctx.ae1_wp_step(feats[0], batches[0], enc_tokens=batches[0], dropout=b.Dropout(1, 0.5, 123, 0))
    elif a.resident:
        loss = ctx.ae_step_rows(rows[0], b.Dropout(1, 0.5, 123, 0))
    else:
        loss = ctx.ae_step(batches[0], b.Dropout(1, 0.5, 123, 0))
    # profiled pass (events around every launch group: slower, reported per group only)
    nprof = 5

    def profiled(c):
        c.profile_enable(True)
        for _ in range(3):
            one_step(c)
        c.sync()
        c.profile_reset()
        for _ in range(nprof):
            one_step(c)
        c.sync()
        out = {k: {"ms_per_step": v["ms"] / nprof, "launches_per_step": v["launches"] / nprof,
                   "tflops": (v["flops"] / (v["ms"] * 1e-3) / 1e12) if v["flops"] > 0 and v["ms"] > 0 else None,
                   "gb_s": (v["bytes"] / (v["ms"] * 1e-3) / 1e9) if v["bytes"] > 0 and v["ms"] > 0 else None}
               for k, v in c.profile().items() if v["launches"] > 0}
        c.profile_enable(False)
        return out

    prof = profiled(ctx)
    world_part = {}
    if ctxw:
        msw = float(np.median(block_ms_world))
        world_part = {"world": a.world, "comm_library": ctxw.comm_library(), "ms_per_step_world": round(msw, 4),
                      "block_ms_world": [round(x, 4) for x in block_ms_world],
                      "exchange_exposed_ms": round(msw - ms, 4),
                      "exchanged_mbytes_per_step": round(4e-6 * ctxw.param_count, 2),
                      "loss_world": ctxw.ae_step(batches[0], b.Dropout(1, 0.5, 123, 0)), "profile_world": profiled(ctxw)}
        ctxw.close()
    ctx.close()
    tmaxes = [int(np.nonzero(t.any(0))[0][-1]) + 1 for t in batches]
    if a.arch == 5:  # the timed steps' own batches and encoder lengths
        fl = float(np.mean([step_flops(a.B, tmaxes[i % len(batches)], a.V, a.E, a.R, a.L, 5,
                                       te=2 if null[i % null.size] else tmaxes[i % len(batches)] + 2, I=I) for i in timed]))
    elif a.arch == 6:
        fl = float(np.mean([step_flops(a.B, tmaxes[i % len(batches)], a.V, a.E, a.R, a.L, 6,
                                       te=0 if null[i % null.size] else tmaxes[i % len(batches)], I=I) for i in timed]))
    else:
        fl = float(np.mean([step_flops(a.B, T, a.V, a.E, a.R, a.L, a.arch) for T in tmaxes]))
    line = {"workload": "ae_arch%d_%s" % (a.arch, "weakpaired" if a.arch in (5, 6) else "text"), "B": a.B, "D": a.D, "V": a.V,
            "E": a.E, "R": a.R, "L": a.L, "ms_per_step": round(ms, 4), "block_ms": [round(x, 4) for x in block_ms],
            "block_spread_pct": round(100.0 * (max(block_ms) - min(block_ms)) / ms, 2),
            "sentences_per_s": round(a.B / (ms * 1e-3), 1), "loss": loss,
            "tflop_per_step": round(fl / 1e12, 4), "achieved_tflops": round(fl / (ms * 1e-3) / 1e12, 2),
            "fraction_of_f32_mfma_peak": round(fl / (ms * 1e-3) / 1e12 / FP32_MFMA_PEAK_TFLOPS, 4),
            "profile": prof}
    line.update(world_part)
    if a.bf16:
        line.update(bf16=1, fraction_of_bf16_mfma_peak=round(fl / (ms * 1e-3) / 1e12 / BF16_MFMA_PEAK_TFLOPS, 4))
    if a.resident:
        line.update(resident=1)
    if a.optim != "adam":
        line.update(optim=a.optim)
    if a.arch in (5, 6):
        line.update(I=I, null_share=a.null_share, null_steps_timed=int(sum(null[i % null.size] for i in timed)))
    s = json.dumps(line)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s + "\n")


if __name__ == "__main__":
    main()
