"""ctypes binding of libnvqa.so (include/nvqa.h) -- the executable twin of
novel-vqa_amd/lua/nvqa_ffi.lua (LuaJIT is not available in the build image).

There is NO fallback: if the shared library or a HIP device is missing the
calls raise NvqaError (the product path never routes through the CPU oracle).
"""
import ctypes
import os

import numpy as np

_PKG = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB_PATH = os.path.join(_PKG, "libnvqa.so")

COMM_ID_BYTES = 128


ARCH1, ARCH2, ARCH_AE1, ARCH_AE2, ARCH_AE2_WP, ARCH_AE1_WP = 1, 2, 3, 4, 5, 6
# NVQA_OPT_*: the update rules of misc/optim_updates.lua (Context.optim_update, Context.ae_wp_projection_update)
OPT_SGD, OPT_SGDM, OPT_SGDMOM, OPT_ADAGRAD, OPT_RMSPROP, OPT_ADAM = 0, 1, 2, 3, 4, 5
# the scripts' -optim / -cnn_optim names
OPT_RULES = {"sgd": OPT_SGD, "sgdm": OPT_SGDM, "sgdmom": OPT_SGDMOM, "adagrad": OPT_ADAGRAD, "rmsprop": OPT_RMSPROP,
             "adam": OPT_ADAM}
CNN_OPT_RULES = {k: OPT_RULES[k] for k in ("sgd", "sgdm", "adam")}


class NvqaError(RuntimeError):
    pass


class Dims(ctypes.Structure):
    """nvqa_dims"""

    _fields_ = [(n, ctypes.c_int32) for n in ("arch", "B", "T", "V", "E", "R", "L", "I", "C", "A")]


class Dropout(ctypes.Structure):
    """nvqa_dropout"""

    _fields_ = [("mode", ctypes.c_int32), ("p", ctypes.c_float), ("seed", ctypes.c_uint64),
                ("step", ctypes.c_uint64)]


class SampleOpts(ctypes.Structure):
    """nvqa_sample_opts: mode SAMPLE_ARGMAX | SAMPLE_MULTINOMIAL | SAMPLE_BEAM; beam_size (beam: 1..8), temperature (multinomial:
    > 0), seed / step (multinomial: keys of the counter-based generator, site NVQA_SITE_AE_SAMPLE)."""

    _fields_ = [("mode", ctypes.c_int32), ("beam_size", ctypes.c_int32), ("temperature", ctypes.c_float),
                ("pad_", ctypes.c_int32), ("seed", ctypes.c_uint64), ("step", ctypes.c_uint64)]


SAMPLE_ARGMAX, SAMPLE_MULTINOMIAL, SAMPLE_BEAM = 0, 1, 2


# every symbol include/nvqa.h declares: name -> (restype, argtypes)
_vp, _i32p, _f32p = ctypes.c_void_p, ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_float)
_i64p = ctypes.POINTER(ctypes.c_int64)
_u8p = ctypes.POINTER(ctypes.c_uint8)
SYMBOLS = {
    "nvqa_create": (ctypes.c_int, [ctypes.POINTER(Dims), ctypes.c_int, ctypes.POINTER(_vp)]),
    "nvqa_destroy": (ctypes.c_int, [_vp]),
    "nvqa_last_error": (ctypes.c_char_p, []),
    "nvqa_sync": (ctypes.c_int, [_vp]),
    "nvqa_param_count": (ctypes.c_size_t, [_vp]),
    "nvqa_segments": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_size_t)]),
    "nvqa_init_params": (ctypes.c_int, [_vp, ctypes.c_uint64, ctypes.c_float, ctypes.c_float]),
    "nvqa_set_params": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_get_params": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_get_grads": (ctypes.c_int, [_vp, _f32p, ctypes.c_float]),
    "nvqa_step": (ctypes.c_int, [_vp, _i32p, _i32p, _f32p, _i32p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_get_loss": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_forward": (ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _i32p, _f32p, _f32p, _i32p]),
    "nvqa_evaluate": (ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _i32p, _f32p, _i32p, _i32p, ctypes.c_int32, _f32p, _i32p,
                                     _i32p, _f32p]),
    "nvqa_rmsprop_update": (ctypes.c_int, [_vp] + [ctypes.c_float] * 5),
    "nvqa_set_fusion": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_set_precision": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_set_ref_quirks": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_param_norms": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_persistent_state": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int)]),
    "nvqa_wgrad_routes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "nvqa_dx0_routes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "nvqa_set_grad_scales": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_dataset_load": (ctypes.c_int, [_vp, ctypes.c_int64, _i32p, _i32p, _i32p, _i32p,
                                         ctypes.c_int64, _f32p, ctypes.c_int]),
    "nvqa_step_indices": (ctypes.c_int, [_vp, _i64p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_comm_unique_id": (ctypes.c_int, [_vp]),
    "nvqa_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "nvqa_comm_library": (ctypes.c_char_p, []),
    "nvqa_vgg16_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.POINTER(_vp)]),
    "nvqa_vgg16_destroy": (ctypes.c_int, [_vp]),
    "nvqa_vgg16_weight_count": (ctypes.c_size_t, [_vp]),
    "nvqa_vgg16_feature_dim": (ctypes.c_int, [_vp]),
    "nvqa_vgg16_set_weights": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_vgg16_fc7": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, _f32p]),
    "nvqa_vgg16_set_precision": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_vgg16_preprocess": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_int, ctypes.c_int, _f32p]),
    "nvqa_vgg16_fc7_raw": (ctypes.c_int, [_vp, _u8p] + [ctypes.c_int] * 4 + [ctypes.POINTER(Dropout), _f32p]),
    "nvqa_vgg16_train_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_vgg16_train_forward_raw": (ctypes.c_int, [_vp, _u8p] + [ctypes.c_int] * 4 + [ctypes.POINTER(Dropout), _f32p]),
    "nvqa_vgg16_train_activation": (ctypes.c_int, [_vp, ctypes.c_int, _f32p]),
    "nvqa_vgg16_backward": (ctypes.c_int, [_vp, _f32p, ctypes.c_int, ctypes.c_int]),
    "nvqa_vgg16_get_grads": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_vgg16_get_weights": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_vgg16_update": (ctypes.c_int, [_vp, ctypes.c_int] + [ctypes.c_float] * 7 + [_f32p]),
    "nvqa_step_images": (ctypes.c_int, [_vp, _vp, _f32p, _i32p, _i32p, _i32p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae_step": (ctypes.c_int, [_vp, _i32p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae_evaluate": (ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _f32p, _i32p]),
    "nvqa_ae_step_images": (ctypes.c_int, [_vp, _f32p, _i32p, ctypes.POINTER(Dropout), _f32p, _f32p]),
    "nvqa_ae_evaluate_images": (ctypes.c_int, [_vp, ctypes.c_int32, _f32p, _i32p, _f32p, _i32p]),
    "nvqa_ae_set_precision": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_ae_comm_init": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, _vp]),
    "nvqa_ae_corpus_load": (ctypes.c_int, [_vp, ctypes.c_int64, _i32p]),
    "nvqa_ae_step_rows": (ctypes.c_int, [_vp, _i64p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae_evaluate_rows": (ctypes.c_int, [_vp, ctypes.c_int32, _i64p, _f32p, _i32p]),
    "nvqa_ae_step_routes": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int64)]),
    "nvqa_ae_sample": (ctypes.c_int, [_vp, ctypes.c_int32, _f32p, _i32p, ctypes.POINTER(SampleOpts), _i32p, _f32p]),
    "nvqa_ae_sample_rows": (ctypes.c_int, [_vp, ctypes.c_int32, _i64p, ctypes.POINTER(SampleOpts), _i32p, _f32p]),
    "nvqa_adam_update": (ctypes.c_int, [_vp] + [ctypes.c_float] * 6 + [_f32p]),
    "nvqa_optim_update": (ctypes.c_int, [_vp, ctypes.c_int] + [ctypes.c_float] * 6 + [_f32p]),
    "nvqa_ae_wp_step": (ctypes.c_int, [_vp, _f32p, _i32p, _i32p, ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae_wp_step_dfeats": (ctypes.c_int, [_vp, _f32p, _i32p, _i32p, ctypes.POINTER(Dropout), _f32p, _f32p]),
    "nvqa_ae_wp_step_images_finetune": (ctypes.c_int, [_vp, _vp, _u8p] + [ctypes.c_int] * 3 + [ctypes.POINTER(Dropout), _i32p, _i32p,
                                                       ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae1_wp_step_images_finetune": (ctypes.c_int, [_vp, _vp, _u8p] + [ctypes.c_int] * 3 + [ctypes.POINTER(Dropout), _i32p, _f32p, _i32p,
                                                        ctypes.POINTER(Dropout), _f32p, _f32p]),
    "nvqa_ae_wp_evaluate": (ctypes.c_int, [_vp, ctypes.c_int32, _f32p, _i32p, _i32p, _f32p, _i32p]),
    "nvqa_ae_wp_set_projection": (ctypes.c_int, [_vp, _f32p, _f32p]),
    "nvqa_ae_wp_get_projection": (ctypes.c_int, [_vp, _f32p, _f32p]),
    "nvqa_ae_wp_get_projection_grads": (ctypes.c_int, [_vp, _f32p, _f32p]),
    "nvqa_ae_wp_projection_adam": (ctypes.c_int, [_vp] + [ctypes.c_float] * 6 + [_f32p]),
    "nvqa_ae_wp_projection_update": (ctypes.c_int, [_vp, ctypes.c_int] + [ctypes.c_float] * 6 + [_f32p]),
    "nvqa_ae1_wp_step": (ctypes.c_int, [_vp, _f32p, _i32p, _f32p, _i32p, ctypes.POINTER(Dropout), _f32p, _f32p]),
    "nvqa_ae1_wp_evaluate": (ctypes.c_int, [_vp, ctypes.c_int32, _f32p, _i32p, _i32p, _f32p, _i32p]),
    "nvqa_ae1_wp_encode": (ctypes.c_int, [_vp, ctypes.c_int32, _i32p, _f32p]),
    "nvqa_ae1_wp_set_lookup": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_ae1_wp_get_lookup": (ctypes.c_int, [_vp, _f32p]),
    "nvqa_ae_wp_step_images": (ctypes.c_int, [_vp, _vp, _u8p] + [ctypes.c_int] * 3 + [ctypes.POINTER(Dropout), _i32p, _i32p,
                                              ctypes.POINTER(Dropout), _f32p]),
    "nvqa_ae_wp_evaluate_images": (ctypes.c_int, [_vp, _vp, ctypes.c_int32, _u8p] + [ctypes.c_int] * 3
                                   + [ctypes.POINTER(Dropout), _i32p, _i32p, _f32p, _i32p]),
    "nvqa_ae1_wp_step_images": (ctypes.c_int, [_vp, _vp, _u8p] + [ctypes.c_int] * 3 + [ctypes.POINTER(Dropout), _i32p, _f32p, _i32p,
                                               ctypes.POINTER(Dropout), _f32p, _f32p]),
    "nvqa_ae1_wp_evaluate_images": (ctypes.c_int, [_vp, _vp, ctypes.c_int32, _u8p] + [ctypes.c_int] * 3
                                    + [ctypes.POINTER(Dropout), _i32p, _i32p, _f32p, _i32p]),
    "nvqa_profile_enable": (ctypes.c_int, [_vp, ctypes.c_int]),
    "nvqa_profile_reset": (ctypes.c_int, [_vp]),
    "nvqa_profile_count": (ctypes.c_int, [_vp]),
    "nvqa_profile_name": (ctypes.c_char_p, [_vp, ctypes.c_int]),
    "nvqa_profile_get": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_int64),
                                        ctypes.POINTER(ctypes.c_double),
                                        ctypes.POINTER(ctypes.c_double)]),
}

_lib = None


def load_library(path=None):
    """dlopen libnvqa.so and bind every declared symbol. Raises NvqaError if absent."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    p = path or LIB_PATH
    if not os.path.exists(p):
        raise NvqaError(f"{p} not found: build it with __graft_entry__.build() "
                        f"(make -C novel-vqa_amd); there is no CPU fallback")
    lib = ctypes.CDLL(p)
    for name, (res, args) in SYMBOLS.items():
        fn = getattr(lib, name)  # AttributeError if the symbol is not exported
        fn.restype = res
        fn.argtypes = args
    if path is None:
        _lib = lib
    return lib


def _f32(a):
    return None if a is None else a.ctypes.data_as(_f32p)


def _i32(a):
    return None if a is None else a.ctypes.data_as(_i32p)


def _u8(a):
    return None if a is None else a.ctypes.data_as(_u8p)


def _images_u8(images, n=None):
    """uint8 planar RGB [n x 3 x S x S] as /images/<split> stores it -> (contiguous array, S); no silent conversion"""
    x = np.asarray(images)
    if x.dtype != np.uint8:
        raise ValueError(f"raw images must be uint8 (got {x.dtype}): the float route is Vgg16.fc7")
    if x.ndim != 4 or x.shape[1] != 3 or x.shape[2] != x.shape[3] or (n is not None and x.shape[0] != n):
        raise ValueError(f"raw images must be [{'n' if n is None else n} x 3 x S x S] (got {x.shape})")
    return np.ascontiguousarray(x), int(x.shape[2])


class Context:
    """Owns one nvqa_ctx (one device)."""

    def __init__(self, dims, device=0):
        self.lib = load_library()
        self.dims = dims
        self.fusion = 0  # netdef.AxB until set_fusion says otherwise
        self._h = _vp()
        self._check(self.lib.nvqa_create(ctypes.byref(dims), device, ctypes.byref(self._h)))

    def _check(self, rc):
        if rc != 0:
            raise NvqaError(f"libnvqa error {rc}: {self.lib.nvqa_last_error().decode()}")

    def close(self):
        if self._h:
            self.lib.nvqa_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # ---- parameters -------------------------------------------------------
    @property
    def param_count(self):
        return int(self.lib.nvqa_param_count(self._h))

    def segments(self):
        out = (ctypes.c_size_t * 3)()
        self._check(self.lib.nvqa_segments(self._h, out))
        return tuple(int(x) for x in out)

    def init_params(self, seed=123, lo=-0.08, hi=0.08):
        self._check(self.lib.nvqa_init_params(self._h, seed, lo, hi))

    def set_params(self, params):
        p = np.ascontiguousarray(params, np.float32)
        assert p.size == self.param_count
        self._check(self.lib.nvqa_set_params(self._h, _f32(p)))

    def get_params(self):
        out = np.empty(self.param_count, np.float32)
        self._check(self.lib.nvqa_get_params(self._h, _f32(out)))
        return out

    def get_grads(self, clamp=0.0):
        out = np.empty(self.param_count, np.float32)
        self._check(self.lib.nvqa_get_grads(self._h, _f32(out), clamp))
        return out

    # ---- hot path ------------------------------------------------------------
    def step(self, tokens, lengths, img, labels, dropout=None, want_loss=True):
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        img = np.ascontiguousarray(img, np.float32).reshape(d.B, d.I)
        labels = np.ascontiguousarray(labels, np.int32)
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_step(self._h, _i32(tokens), _i32(lengths), _f32(img), _i32(labels),
                                       dr, ctypes.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def step_indices(self, qinds, dropout=None, want_loss=True):
        q = np.ascontiguousarray(qinds, np.int64)
        assert q.size == self.dims.B
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_step_indices(self._h, q.ctypes.data_as(_i64p), dr,
                                               ctypes.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def step_images(self, vgg, images, tokens, lengths, labels, dropout=None):
        """Extractor + training step in one call (features stay on the device)."""
        d = self.dims
        images = np.ascontiguousarray(images, np.float32)
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        labels = np.ascontiguousarray(labels, np.int32)
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_step_images(self._h, vgg._h, _f32(images), _i32(tokens), _i32(lengths),
                                              _i32(labels), dr, ctypes.byref(loss)))
        return float(loss.value)

    def get_loss(self):
        loss = ctypes.c_float(0)
        self._check(self.lib.nvqa_get_loss(self._h, ctypes.byref(loss)))
        return float(loss.value)

    def forward(self, tokens, lengths, img):
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32)
        n = tokens.shape[0]
        lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        img = np.ascontiguousarray(img, np.float32)
        scores = np.empty((n, d.A), np.float32)
        argmax = np.empty(n, np.int32)
        self._check(self.lib.nvqa_forward(self._h, n, _i32(tokens), _i32(lengths), _f32(img),
                                          _f32(scores), _i32(argmax)))
        return scores, argmax

    def evaluate(self, tokens, lengths, img, labels=None, mc_ans=None):
        """nvqa_evaluate: dict(scores, argmax, loss (if labels), mc_argmax (if mc_ans [n, n_mc], 0 = empty slot))."""
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32)
        n = tokens.shape[0]
        lengths = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        img = np.ascontiguousarray(img, np.float32)
        labels = None if labels is None else np.ascontiguousarray(labels, np.int32)
        mc = None if mc_ans is None else np.ascontiguousarray(mc_ans, np.int32)
        scores = np.empty((n, d.A), np.float32)
        argmax = np.empty(n, np.int32)
        mcout = np.empty(n, np.int32) if mc is not None else None
        loss = ctypes.c_float(0)
        self._check(self.lib.nvqa_evaluate(self._h, n, _i32(tokens), _i32(lengths), _f32(img), _i32(labels), _i32(mc),
                                           0 if mc is None else mc.shape[1], _f32(scores), _i32(argmax), _i32(mcout),
                                           ctypes.byref(loss) if labels is not None else None))
        out = {"scores": scores, "argmax": argmax}
        if labels is not None:
            out["loss"] = float(loss.value)
        if mc is not None:
            out["mc_argmax"] = mcout
        return out

    def rmsprop_update(self, lr, alpha=0.99, eps=1e-8, wd=0.0, clamp=10.0):
        self._check(self.lib.nvqa_rmsprop_update(self._h, lr, alpha, eps, wd, clamp))

    # ---- text auto-encoders (arch ARCH_AE1 / ARCH_AE2) and Adam ---------------------
    def ae_step(self, tokens, dropout=None, want_loss=True, images=None, want_dimages=False):
        """nvqa_ae_step: tokens [B x D] left-aligned, 0 = null.  Returns the criterion's loss (or None).
        ARCH_AE2 only: images [B x E] (None = zeros) and want_dimages go through nvqa_ae_step_images; with
        want_dimages the return value is (loss or None, d(images) [B x E])."""
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        lp = ctypes.byref(loss) if want_loss else None
        if images is None and not want_dimages:
            self._check(self.lib.nvqa_ae_step(self._h, _i32(tokens), dr, lp))
            return float(loss.value) if want_loss else None
        img = None if images is None else np.ascontiguousarray(images, np.float32).reshape(d.B, d.E)
        dimg = np.empty((d.B, d.E), np.float32) if want_dimages else None
        self._check(self.lib.nvqa_ae_step_images(self._h, _f32(img), _i32(tokens), dr, lp, _f32(dimg)))
        out = float(loss.value) if want_loss else None
        return (out, dimg) if want_dimages else out

    def ae_evaluate(self, tokens, samples=False, images=None):
        """nvqa_ae_evaluate: (evaluate-mode loss, greedy samples [n x D] 1-based with V+1 = END, or None).
        ARCH_AE2 only: images [n x E] (None = zeros) go through nvqa_ae_evaluate_images."""
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tokens.shape[0]
        out = np.empty((n, d.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        if images is None:
            self._check(self.lib.nvqa_ae_evaluate(self._h, n, _i32(tokens), ctypes.byref(loss), _i32(out)))
        else:
            img = np.ascontiguousarray(images, np.float32).reshape(n, d.E)
            self._check(self.lib.nvqa_ae_evaluate_images(self._h, n, _f32(img), _i32(tokens), ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def ae_set_precision(self, bf16):
        """nvqa_ae_set_precision: 1 = both operands of every dense product of the ARCH_AE1 / ARCH_AE2 step rounded to bf16,
        f32 accumulate; 0 = f32.  (set_precision(1) stays refused on an auto-encoder context; this one is refused on the
        weak-paired and the VQA contexts.)"""
        self._check(self.lib.nvqa_ae_set_precision(self._h, int(bf16)))

    def ae_comm_init(self, rank, world, comm_id):
        """nvqa_ae_comm_init: data parallel for an ARCH_AE1 / ARCH_AE2 context; comm_id from comm_unique_id() of rank 0.
        Afterwards ae_step ends with the global batch's gradient and loss, the ranks' gradients weighted by their criterion
        counts (comm_init stays refused on an auto-encoder context; this one is refused on the weak-paired and VQA contexts)."""
        buf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._check(self.lib.nvqa_ae_comm_init(self._h, rank, world, ctypes.cast(buf, _vp)))

    def ae_corpus_load(self, tokens):
        """nvqa_ae_corpus_load: tokens [N x D] (0..V, 0 = null, left-aligned) become the context's resident corpus in HBM
        (ARCH_AE1 / ARCH_AE2).  A failed load leaves the previous corpus in place."""
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1, self.dims.T)
        self._check(self.lib.nvqa_ae_corpus_load(self._h, tok.shape[0], _i32(tok)))

    def ae_step_rows(self, rows, dropout=None, want_loss=True):
        """nvqa_ae_step_rows: ae_step on rows [B] (0-based, any order, repeats allowed) of the resident corpus, bit for bit.
        With want_loss=False (and no communicator) the call only enqueues."""
        r = np.ascontiguousarray(rows, np.int64).reshape(-1)
        assert r.size == self.dims.B
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_ae_step_rows(self._h, r.ctypes.data_as(_i64p), dr, ctypes.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def ae_evaluate_rows(self, rows, samples=False):
        """nvqa_ae_evaluate_rows: ae_evaluate on n = len(rows) <= B rows of the resident corpus."""
        r = np.ascontiguousarray(rows, np.int64).reshape(-1)
        n = r.size
        out = np.empty((n, self.dims.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        self._check(self.lib.nvqa_ae_evaluate_rows(self._h, n, r.ctypes.data_as(_i64p), ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def ae_sample(self, tokens, opts=None, images=None, logprobs=False):
        """nvqa_ae_sample: decode n = len(tokens) <= B rows by opts (SampleOpts; None = argmax).  Returns seq [n x D] (1-based,
        V+1 = END; beam: zeros behind END), or (seq, log-probabilities [n x D] of the emitted tokens) with logprobs=True.
        ARCH_AE2 only: images [n x E] (None = zeros)."""
        d = self.dims
        tokens = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tokens.shape[0]
        img = None if images is None else np.ascontiguousarray(images, np.float32).reshape(n, d.E)
        seq = np.empty((n, d.T), np.int32)
        lp = np.empty((n, d.T), np.float32) if logprobs else None
        self._check(self.lib.nvqa_ae_sample(self._h, n, _f32(img), _i32(tokens), ctypes.byref(opts) if opts is not None else None,
                                            _i32(seq), _f32(lp)))
        return (seq, lp) if logprobs else seq

    def ae_sample_rows(self, rows, opts=None, logprobs=False):
        """nvqa_ae_sample_rows: ae_sample on n = len(rows) <= B rows of the resident corpus."""
        r = np.ascontiguousarray(rows, np.int64).reshape(-1)
        n = r.size
        seq = np.empty((n, self.dims.T), np.int32)
        lp = np.empty((n, self.dims.T), np.float32) if logprobs else None
        self._check(self.lib.nvqa_ae_sample_rows(self._h, n, r.ctypes.data_as(_i64p), ctypes.byref(opts) if opts is not None else None,
                                                 _i32(seq), _f32(lp)))
        return (seq, lp) if logprobs else seq

    def ae_step_routes(self):
        """Training steps so far by where their batch came from: {'host': ae_step*, 'resident': ae_step_rows}."""
        out = (ctypes.c_int64 * 2)()
        self._check(self.lib.nvqa_ae_step_routes(self._h, out))
        return {"host": int(out[0]), "resident": int(out[1])}

    def adam_update(self, lr, beta1=0.8, beta2=0.999, eps=1e-8, wd=0.0, clamp=0.0, stats=False):
        """clamp -> + wd x -> adam in one pass; stats=True returns (paramsNorm, # updates) of the log line."""
        out = np.zeros(2, np.float32) if stats else None
        self._check(self.lib.nvqa_adam_update(self._h, lr, beta1, beta2, eps, wd, clamp, _f32(out)))
        return (float(out[0]), int(out[1])) if stats else None

    def optim_update(self, rule, lr, alpha=0.8, beta=0.999, eps=1e-8, wd=0.0, clamp=0.0, stats=False):
        """nvqa_optim_update: clamp -> + wd x -> the rule (OPT_SGD .. OPT_ADAM, misc/optim_updates.lua) in one pass, on any
        context; stats=True returns (paramsNorm, # updates) of the log line.  OPT_RMSPROP shares rmsprop_update's state and
        bits, OPT_ADAM adam_update's."""
        out = np.zeros(2, np.float32) if stats else None
        self._check(self.lib.nvqa_optim_update(self._h, int(rule), lr, alpha, beta, eps, wd, clamp, _f32(out)))
        return (float(out[0]), int(out[1])) if stats else None

    # ---- weak-paired auto-encoder (arch ARCH_AE2_WP) --------------------------------
    def ae_wp_step(self, feats, tokens, enc_tokens=None, dropout=None, want_loss=True, want_dfeats=False):
        """nvqa_ae_wp_step: feats [B x I] (the frozen CNN body's output; the library L2-normalises its copy), tokens [B x D]
        for the decoder and criterion, enc_tokens [B x D] for the encoder (None = the null sentence).  want_dfeats:
        nvqa_ae_wp_step_dfeats, returning (loss, d(loss)/d(f^) [B x I])."""
        d = self.dims
        f = np.ascontiguousarray(feats, np.float32).reshape(d.B, d.I)
        tok = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(d.B, d.T)
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        if want_dfeats:
            df = np.empty((d.B, d.I), np.float32)
            self._check(self.lib.nvqa_ae_wp_step_dfeats(self._h, _f32(f), _i32(et), _i32(tok), dr,
                                                        ctypes.byref(loss) if want_loss else None, _f32(df)))
            return (float(loss.value) if want_loss else None), df
        self._check(self.lib.nvqa_ae_wp_step(self._h, _f32(f), _i32(et), _i32(tok), dr, ctypes.byref(loss) if want_loss else None))
        return float(loss.value) if want_loss else None

    def ae_wp_evaluate(self, feats, tokens, enc_tokens=None, samples=False):
        """nvqa_ae_wp_evaluate of n = len(tokens) rows: (evaluate-mode loss, greedy samples [n x D] or None)."""
        d = self.dims
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tok.shape[0]
        f = np.ascontiguousarray(feats, np.float32).reshape(n, d.I)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(n, d.T)
        out = np.empty((n, d.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        self._check(self.lib.nvqa_ae_wp_evaluate(self._h, n, _f32(f), _i32(et), _i32(tok), ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def ae_wp_set_projection(self, w, b):
        d = self.dims
        w = np.ascontiguousarray(w, np.float32).reshape(d.E, d.I)
        b = np.ascontiguousarray(b, np.float32).reshape(d.E)
        self._check(self.lib.nvqa_ae_wp_set_projection(self._h, _f32(w), _f32(b)))

    def ae_wp_get_projection(self):
        """(W_p [E x I], b_p [E])"""
        d = self.dims
        w, b = np.empty((d.E, d.I), np.float32), np.empty(d.E, np.float32)
        self._check(self.lib.nvqa_ae_wp_get_projection(self._h, _f32(w), _f32(b)))
        return w, b

    def ae_wp_get_projection_grads(self):
        """(dW_p [E x I], db_p [E]) of the last step"""
        d = self.dims
        w, b = np.empty((d.E, d.I), np.float32), np.empty(d.E, np.float32)
        self._check(self.lib.nvqa_ae_wp_get_projection_grads(self._h, _f32(w), _f32(b)))
        return w, b

    def ae_wp_projection_adam(self, lr, beta1=0.8, beta2=0.999, eps=1e-8, wd=0.0, clamp=0.0, stats=False):
        """+ wd x -> clamp -> adam on [W_p | b_p]; stats=True returns (||W_p||, # cnn updates) of the log line."""
        out = np.zeros(2, np.float32) if stats else None
        self._check(self.lib.nvqa_ae_wp_projection_adam(self._h, lr, beta1, beta2, eps, wd, clamp, _f32(out)))
        return (float(out[0]), int(out[1])) if stats else None

    def ae_wp_projection_update(self, rule, lr, alpha=0.8, beta=0.999, eps=1e-8, wd=0.0, clamp=0.0, stats=False):
        """nvqa_ae_wp_projection_update: + wd x -> clamp -> OPT_SGD | OPT_SGDM | OPT_ADAM on [W_p | b_p] (-cnn_optim);
        stats as ae_wp_projection_adam, whose state and bits OPT_ADAM shares."""
        out = np.zeros(2, np.float32) if stats else None
        self._check(self.lib.nvqa_ae_wp_projection_update(self._h, int(rule), lr, alpha, beta, eps, wd, clamp, _f32(out)))
        return (float(out[0]), int(out[1])) if stats else None

    # ---- arch1 weak-paired auto-encoder (arch ARCH_AE1_WP) --------------------------
    def ae1_wp_step(self, feats, tokens, enc_tokens=None, enc_state=None, dropout=None, want_loss=True, want_dfeats=False):
        """nvqa_ae1_wp_step: feats [B x I], tokens [B x D] for the decoder and criterion, and exactly one of enc_tokens [B x D]
        (the encoder runs) and enc_state [B x 2R] (encoder_skip_flag = 1).  Returns the loss (or None); with want_dfeats
        (loss or None, d(loss)/d(f^) [B x I])."""
        d = self.dims
        f = np.ascontiguousarray(feats, np.float32).reshape(d.B, d.I)
        tok = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(d.B, d.T)
        es = None if enc_state is None else np.ascontiguousarray(enc_state, np.float32).reshape(d.B, 2 * d.R)
        df = np.empty((d.B, d.I), np.float32) if want_dfeats else None
        loss = ctypes.c_float(0)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_ae1_wp_step(self._h, _f32(f), _i32(et), _f32(es), _i32(tok), dr,
                                              ctypes.byref(loss) if want_loss else None, _f32(df)))
        out = float(loss.value) if want_loss else None
        return (out, df) if want_dfeats else out

    def ae1_wp_evaluate(self, feats, tokens, enc_tokens, samples=False):
        """nvqa_ae1_wp_evaluate of n = len(tokens) rows: (evaluate-mode loss, greedy samples [n x D] or None)."""
        d = self.dims
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tok.shape[0]
        f = np.ascontiguousarray(feats, np.float32).reshape(n, d.I)
        et = np.ascontiguousarray(enc_tokens, np.int32).reshape(n, d.T)
        out = np.empty((n, d.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        self._check(self.lib.nvqa_ae1_wp_evaluate(self._h, n, _f32(f), _i32(et), _i32(tok), ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def ae1_wp_encode(self, enc_tokens):
        """nvqa_ae1_wp_encode: the evaluate-mode [c_T | h_T] [n x 2R] of n = len(enc_tokens) <= B rows."""
        d = self.dims
        et = np.ascontiguousarray(enc_tokens, np.int32).reshape(-1, d.T)
        out = np.empty((et.shape[0], 2 * d.R), np.float32)
        self._check(self.lib.nvqa_ae1_wp_encode(self._h, et.shape[0], _i32(et), _f32(out)))
        return out

    def ae1_wp_set_lookup(self, w):
        d = self.dims
        w = np.ascontiguousarray(w, np.float32).reshape(d.V + 1, d.E)
        self._check(self.lib.nvqa_ae1_wp_set_lookup(self._h, _f32(w)))

    def ae1_wp_get_lookup(self):
        """the frozen W_lk [(V+1) x E]"""
        d = self.dims
        w = np.empty((d.V + 1, d.E), np.float32)
        self._check(self.lib.nvqa_ae1_wp_get_lookup(self._h, _f32(w)))
        return w

    # ---- the weak-paired steps with the VGG-16 body in the loop -----------------------
    def ae_wp_step_images(self, vgg, images_u8, xoff, yoff, tokens, enc_tokens=None, body_dropout=None, dropout=None,
                          want_loss=True, finetune=False):
        """nvqa_ae_wp_step_images: ae_wp_step fed by the extractor `vgg` (Vgg16) on images_u8 [B x 3 x S x S] uint8, window
        origin (xoff, yoff), body_dropout (Dropout or None: drop6 / drop7 off).  The features stay on the device; with
        want_loss=False the call only enqueues."""
        d = self.dims
        x, S = _images_u8(images_u8, d.B)
        tok = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(d.B, d.T)
        loss = ctypes.c_float(0)
        bdr = ctypes.byref(body_dropout) if body_dropout is not None else None
        dr = ctypes.byref(dropout) if dropout is not None else None
        # finetune: nvqa_ae_wp_step_images_finetune -- a training-enabled extractor also gets its gradients (vgg.get_grads)
        fn = self.lib.nvqa_ae_wp_step_images_finetune if finetune else self.lib.nvqa_ae_wp_step_images
        self._check(fn(self._h, vgg._h, _u8(x), S, int(xoff), int(yoff), bdr, _i32(et), _i32(tok), dr,
                                                    ctypes.byref(loss) if want_loss else None))
        if finetune:
            vgg._train_n = d.B
        return float(loss.value) if want_loss else None

    def ae_wp_evaluate_images(self, vgg, images_u8, xoff, yoff, tokens, enc_tokens=None, body_dropout=None, samples=False):
        """nvqa_ae_wp_evaluate_images of n = len(tokens) rows: (evaluate-mode loss, greedy samples [n x D] or None)."""
        d = self.dims
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tok.shape[0]
        x, S = _images_u8(images_u8, n)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(n, d.T)
        out = np.empty((n, d.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        bdr = ctypes.byref(body_dropout) if body_dropout is not None else None
        self._check(self.lib.nvqa_ae_wp_evaluate_images(self._h, vgg._h, n, _u8(x), S, int(xoff), int(yoff), bdr, _i32(et), _i32(tok),
                                                        ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def ae1_wp_step_images(self, vgg, images_u8, xoff, yoff, tokens, enc_tokens=None, enc_state=None, body_dropout=None,
                           dropout=None, want_loss=True, want_dfeats=False, finetune=False):
        """nvqa_ae1_wp_step_images: ae1_wp_step fed by the extractor; returns as ae1_wp_step does (dfeats = d(loss)/d(f^))."""
        d = self.dims
        x, S = _images_u8(images_u8, d.B)
        tok = np.ascontiguousarray(tokens, np.int32).reshape(d.B, d.T)
        et = None if enc_tokens is None else np.ascontiguousarray(enc_tokens, np.int32).reshape(d.B, d.T)
        es = None if enc_state is None else np.ascontiguousarray(enc_state, np.float32).reshape(d.B, 2 * d.R)
        df = np.empty((d.B, d.I), np.float32) if want_dfeats else None
        loss = ctypes.c_float(0)
        bdr = ctypes.byref(body_dropout) if body_dropout is not None else None
        dr = ctypes.byref(dropout) if dropout is not None else None
        fn = self.lib.nvqa_ae1_wp_step_images_finetune if finetune else self.lib.nvqa_ae1_wp_step_images
        self._check(fn(self._h, vgg._h, _u8(x), S, int(xoff), int(yoff), bdr, _i32(et), _f32(es),
                       _i32(tok), dr, ctypes.byref(loss) if want_loss else None, _f32(df)))
        if finetune:
            vgg._train_n = d.B
        out = float(loss.value) if want_loss else None
        return (out, df) if want_dfeats else out

    def ae1_wp_evaluate_images(self, vgg, images_u8, xoff, yoff, tokens, enc_tokens, body_dropout=None, samples=False):
        """nvqa_ae1_wp_evaluate_images of n = len(tokens) rows: (evaluate-mode loss, greedy samples [n x D] or None)."""
        d = self.dims
        tok = np.ascontiguousarray(tokens, np.int32).reshape(-1, d.T)
        n = tok.shape[0]
        x, S = _images_u8(images_u8, n)
        et = np.ascontiguousarray(enc_tokens, np.int32).reshape(n, d.T)
        out = np.empty((n, d.T), np.int32) if samples else None
        loss = ctypes.c_float(0)
        bdr = ctypes.byref(body_dropout) if body_dropout is not None else None
        self._check(self.lib.nvqa_ae1_wp_evaluate_images(self._h, vgg._h, n, _u8(x), S, int(xoff), int(yoff), bdr, _i32(et), _i32(tok),
                                                         ctypes.byref(loss), _i32(out)))
        return float(loss.value), out

    def set_fusion(self, mode):
        """0 netdef.AxB, 1 netdef.AskipB, 2 netdef.A_B (W_o becomes [A x 2C]: right after creation only)."""
        self._check(self.lib.nvqa_set_fusion(self._h, int(mode)))
        self.fusion = int(mode)

    QUIRK_H0, QUIRK_LOOKUP = 1, 2

    def set_ref_quirks(self, flags):
        """arch2: reproduce the reference's aliased-h0 / untrained-lookup artefacts (include/nvqa.h)."""
        self._check(self.lib.nvqa_set_ref_quirks(self._h, int(flags)))

    def set_precision(self, bf16):
        self._check(self.lib.nvqa_set_precision(self._h, int(bool(bf16))))

    def set_grad_scales(self, scales):
        a = np.ascontiguousarray(scales, np.float32)
        assert a.size == 3
        self._check(self.lib.nvqa_set_grad_scales(self._h, _f32(a)))

    def sync(self):
        self._check(self.lib.nvqa_sync(self._h))

    def param_norms(self):
        """torch.norm of the three parameter segments (arch2's training log line, 002_train_baseline.lua:400-407)"""
        out = np.empty(3, np.float32)
        self._check(self.lib.nvqa_param_norms(self._h, _f32(out)))
        return out

    def persistent_state(self):
        """{'fwd': bool, 'bwd': bool}: does the next step run the LSTM unroll / the BPTT as one persistent launch?"""
        out = (ctypes.c_int * 2)()
        self._check(self.lib.nvqa_persistent_state(self._h, out))
        return {"fwd": bool(out[0]), "bwd": bool(out[1])}

    def wgrad_routes(self):
        """Weight-gradient products launched so far by route: {'f32_chain', 'split', 'split2'} (NVQA_WGRAD_SPLIT / NVQA_WGRAD_KERNEL)."""
        out = (ctypes.c_int64 * 3)()
        self._check(self.lib.nvqa_wgrad_routes(self._h, out))
        return {"f32_chain": int(out[0]), "split": int(out[1]), "split2": int(out[2])}

    def dx0_routes(self):
        """f32-mode d(layer-0 input) products launched so far by route: {'f32_gemm', 'split'} (NVQA_DX0_KERNEL)."""
        out = (ctypes.c_int64 * 2)()
        self._check(self.lib.nvqa_dx0_routes(self._h, out))
        return {"f32_gemm": int(out[0]), "split": int(out[1])}

    # ---- dataset ------------------------------------------------------------------
    def dataset_load(self, questions, lengths, img_pos, answers, feats, l2_normalize=False):
        q = np.ascontiguousarray(questions, np.int32)
        l = None if lengths is None else np.ascontiguousarray(lengths, np.int32)
        ip = np.ascontiguousarray(img_pos, np.int32)
        an = np.ascontiguousarray(answers, np.int32)
        f = np.ascontiguousarray(feats, np.float32)
        self._check(self.lib.nvqa_dataset_load(self._h, q.shape[0], _i32(q), _i32(l), _i32(ip), _i32(an),
                                               f.shape[0], _f32(f), int(l2_normalize)))

    # ---- data parallel ------------------------------------------------------------
    def comm_unique_id(self):
        buf = ctypes.create_string_buffer(COMM_ID_BYTES)
        self._check(self.lib.nvqa_comm_unique_id(ctypes.cast(buf, _vp)))
        return buf.raw

    def comm_library(self):
        """path of the collective library behind nvqa_comm_* (NVQA_RCCL_LIB, or the librccl beside the mapped HIP runtime)"""
        p = self.lib.nvqa_comm_library()
        if p is None:
            raise NvqaError(f"libnvqa: {self.lib.nvqa_last_error().decode()}")
        return p.decode()

    def comm_init(self, rank, world, comm_id):
        buf = ctypes.create_string_buffer(bytes(comm_id), COMM_ID_BYTES)
        self._check(self.lib.nvqa_comm_init(self._h, rank, world, ctypes.cast(buf, _vp)))

    # ---- measurement ----------------------------------------------------------------
    def profile_enable(self, on=True):
        self._check(self.lib.nvqa_profile_enable(self._h, int(on)))

    def profile_reset(self):
        self._check(self.lib.nvqa_profile_reset(self._h))

    def profile(self):
        out = {}
        for i in range(self.lib.nvqa_profile_count(self._h)):
            ms, n, fl, by = ctypes.c_double(), ctypes.c_int64(), ctypes.c_double(), ctypes.c_double()
            self._check(self.lib.nvqa_profile_get(self._h, i, ctypes.byref(ms), ctypes.byref(n),
                                                  ctypes.byref(fl), ctypes.byref(by)))
            out[self.lib.nvqa_profile_name(self._h, i).decode()] = {
                "ms": ms.value, "launches": n.value, "flops": fl.value, "bytes": by.value}
        return out


class Vgg16:
    """VGG-16 fc7 extractor (001_prepro_img_vgg.lua): owns one nvqa_vgg."""

    def __init__(self, device=0, width_div=1, input_hw=224, max_batch=16):
        self.lib = load_library()
        self._h = _vp()
        self.hw = input_hw
        self.width_div = width_div
        self._check(self.lib.nvqa_vgg16_create(device, width_div, input_hw, max_batch, ctypes.byref(self._h)))
        self.weight_count = int(self.lib.nvqa_vgg16_weight_count(self._h))
        self.feature_dim = int(self.lib.nvqa_vgg16_feature_dim(self._h))

    def _check(self, rc):
        if rc != 0:
            raise NvqaError(f"libnvqa error {rc}: {self.lib.nvqa_last_error().decode()}")

    def set_weights(self, flat):
        w = np.ascontiguousarray(flat, np.float32)
        assert w.size == self.weight_count
        self._check(self.lib.nvqa_vgg16_set_weights(self._h, _f32(w)))

    def set_precision(self, bf16):
        """1 = operands of the convolutions / fc products rounded to bf16 (f32 accumulate, f32 features)"""
        self._check(self.lib.nvqa_vgg16_set_precision(self._h, int(bool(bf16))))

    def fc7(self, images):
        x = np.ascontiguousarray(images, np.float32)
        n = x.shape[0]
        assert x.shape[1:] == (3, self.hw, self.hw)
        out = np.empty((n, self.feature_dim), np.float32)
        self._check(self.lib.nvqa_vgg16_fc7(self._h, _f32(x), n, _f32(out)))
        return out

    def fc7_raw(self, images_u8, xoff, yoff, dropout=None):
        """nvqa_vgg16_fc7_raw: images_u8 [n x 3 x S x S] uint8 planar RGB; the hw x hw window at (xoff, yoff), mean-subtracted,
        through the network.  dropout (Dropout, mode 1): drop6 / drop7 live.  Returns module 38's output [n x F]."""
        x, S = _images_u8(images_u8)
        n = x.shape[0]
        out = np.empty((n, self.feature_dim), np.float32)
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_vgg16_fc7_raw(self._h, _u8(x), n, S, int(xoff), int(yoff), dr, _f32(out)))
        return out

    # ---- fine-tuning (f32 body only) ----
    def train_enable(self, on=True):
        """allocate (True) or free (False) the training state: saved activations, gradients, W', workspace"""
        self._check(self.lib.nvqa_vgg16_train_enable(self._h, int(bool(on))))
        if not on:
            self._train_n = 0  # the saved activations went with the state

    def train_forward_raw(self, images_u8, xoff, yoff, dropout=None, want_feats=True):
        """fc7_raw's arguments and bits, every layer's output kept for backward(); returns the features, or None"""
        x, S = _images_u8(images_u8)
        n = x.shape[0]
        out = np.empty((n, self.feature_dim), np.float32) if want_feats else None
        dr = ctypes.byref(dropout) if dropout is not None else None
        self._check(self.lib.nvqa_vgg16_train_forward_raw(self._h, _u8(x), n, S, int(xoff), int(yoff), dr,
                                                          _f32(out) if want_feats else None))
        self._train_n = n
        return out

    def conv_shape(self, which):
        """(channels, height) of convolution `which`'s output (0..12); the two tables follow kConvCout / kPoolAfter of
        csrc/vgg.hip (the ABI has no call that returns a layer's shape)"""
        cout = [64, 64, 128, 128, 256, 256, 256, 512, 512, 512, 512, 512, 512]
        pools = [0, 1, 0, 1, 0, 0, 1, 0, 0, 1, 0, 0, 1]
        return max(1, cout[which] // self.width_div), self.hw >> sum(pools[:which])

    def train_activation(self, which):
        """saved output of layer 0..12 (convolution, post-ReLU, NCHW), 13 (fc6), 14 (fc7) of the last training forward"""
        n = getattr(self, "_train_n", 0)
        if not n:
            raise NvqaError("train_activation before train_forward_raw")
        if which >= 13:
            out = np.empty((n, self.feature_dim), np.float32)
        else:
            c, h = self.conv_shape(which)
            out = np.empty((n, c, h, h), np.float32)
        self._check(self.lib.nvqa_vgg16_train_activation(self._h, int(which), _f32(out)))
        return out

    def backward(self, dfeats, through_l2norm=False):
        """d(loss)/d(features) [n x F] (through_l2norm: d/d(f^) of the row-normalised features) -> the body's gradients"""
        d = np.ascontiguousarray(dfeats, np.float32)
        assert d.ndim == 2 and d.shape[1] == self.feature_dim
        self._check(self.lib.nvqa_vgg16_backward(self._h, _f32(d), d.shape[0], int(bool(through_l2norm))))

    def get_grads(self):
        out = np.empty(self.weight_count, np.float32)
        self._check(self.lib.nvqa_vgg16_get_grads(self._h, _f32(out)))
        return out

    def get_weights(self):
        out = np.empty(self.weight_count, np.float32)
        self._check(self.lib.nvqa_vgg16_get_weights(self._h, _f32(out)))
        return out

    def update(self, rule, lr, alpha=0.9, beta=0.999, eps=1e-8, wd=0.0, clamp=0.0, scale=1.0, want_stats=True):
        """one -cnn_optim update (OPT_SGD / OPT_SGDM / OPT_ADAM) of every weight of the body; returns (|x|, updates >= 1%)"""
        st = np.zeros(2, np.float32)
        self._check(self.lib.nvqa_vgg16_update(self._h, int(rule), lr, alpha, beta, eps, wd, clamp, scale,
                                               _f32(st) if want_stats else None))
        return (float(st[0]), float(st[1])) if want_stats else None

    def preprocess(self, rgb):
        x = np.ascontiguousarray(rgb, np.float32)
        n, _, H, W = x.shape
        out = np.empty((n, 3, self.hw, self.hw), np.float32)
        self._check(self.lib.nvqa_vgg16_preprocess(self._h, _f32(x), n, H, W, _f32(out)))
        return out

    def close(self):
        if self._h:
            self.lib.nvqa_vgg16_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
