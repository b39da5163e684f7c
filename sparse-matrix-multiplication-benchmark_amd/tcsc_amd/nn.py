"""torch autograd layer over the TCSC device API.

``PackedTernaryLinear`` is the inference-only layer on a packed plan (DESIGN.md
§18): the 2-bit image of ``W`` alone, int8 activations quantized per row.

``TernaryLinear`` computes ``y = act(x . W + b)`` for a frozen ternary ``W``
(K x N) held as a :class:`tcsc_amd.Plan`, and its backward: ``dZ`` and ``db`` by
``tcsc_gpu_prelu_backward``, ``dX = dZ . W^T`` by ``tcsc_gpu_sgemm_t`` on the
transposed plan.  Every launch goes on torch's current stream.

torch is imported lazily, as ``tcsc_amd.lib()`` does: importing this module
needs neither torch nor a GPU; the first access to ``TernaryLinear`` does the
import and defines the classes (a ``torch.nn.Module`` subclass needs torch to
exist).
"""
from __future__ import annotations

import numpy as np

from . import Plan, TcscError, TcscMatrix, prelu_backward, ternarize_absmean, w2_image_bytes

__all__ = ["TernaryLinear", "PackedTernaryLinear", "PackedTernaryGLU", "PackedTernaryMLP", "PackedTernaryGroup"]

_classes = None


def _define():
    import torch

    def _stream(device) -> int:
        return torch.cuda.current_stream(device).cuda_stream

    def _ternary_matrix(W, who: str) -> TcscMatrix:
        """W as the layers take it: a TcscMatrix (kept by reference) or a dense K x N of -1, 0, +1."""
        if isinstance(W, TcscMatrix):
            if not W.ptr:
                raise TcscError(f"{who}: W is a freed TcscMatrix")
            return W
        Wd = W.detach().cpu().numpy() if torch.is_tensor(W) else np.asarray(W)
        if Wd.ndim != 2:
            raise TcscError(f"{who}: W must be 2-D (K x N), got shape {Wd.shape}")
        Wd = np.ascontiguousarray(Wd, dtype=np.float32)
        if not np.isin(Wd, (-1.0, 0.0, 1.0)).all():
            raise TcscError(f"{who}: W must hold only -1, 0 and +1")
        return TcscMatrix.from_dense(Wd)

    def _bias_tensor(bias, n: int, dev, who: str):
        if bias is None:
            return torch.zeros(n, dtype=torch.float32, device=dev)
        b = torch.as_tensor(bias).detach().to(device=dev, dtype=torch.float32).reshape(-1).clone()
        if b.numel() != n:
            raise TcscError(f"{who}: bias has {b.numel()} elements, W has N={n} columns")
        return b

    def _weight_scale_tensor(ws, n: int, dev):
        """None, one float (broadcast) or n values -> None or n contiguous floats on dev."""
        if ws is None:
            return None
        t = torch.as_tensor(ws).detach().to(device=dev, dtype=torch.float32).reshape(-1)
        if t.numel() == 1:
            return t.expand(n).contiguous()
        if t.numel() != n:
            raise TcscError(f"PackedTernaryLinear: weight_scale has {t.numel()} elements, W has N={n} columns "
                            "(one value or one per column)")
        return t.clone()

    def _norm_args(norm_weight, norm_eps, k: int, dev):
        """(norm_weight as None or k contiguous floats on dev, norm_eps as None or a float > 0)."""
        if norm_eps is None:
            if norm_weight is not None:
                raise TcscError("PackedTernaryLinear: norm_weight needs norm_eps (the layer has no norm without it)")
            return None, None
        eps = float(norm_eps)
        if not (eps > 0.0 and eps < float("inf")):
            raise TcscError(f"PackedTernaryLinear: norm_eps must be a finite number > 0, got {norm_eps!r}")
        if norm_weight is None:
            return None, eps
        t = torch.as_tensor(norm_weight).detach().to(device=dev, dtype=torch.float32).reshape(-1).clone()
        if t.numel() != k:
            raise TcscError(f"PackedTernaryLinear: norm_weight has {t.numel()} elements, W has K={k} rows")
        return t, eps

    def _out_dtype(dt):
        if dt not in (torch.float32, torch.bfloat16):
            raise TcscError(f"PackedTernaryLinear: out_dtype must be torch.float32 or torch.bfloat16, got {dt!r}")
        return dt

    class _TernaryLinearFn(torch.autograd.Function):
        """y = act(x . W + b) on an (M x K) contiguous fp32 or bf16 x (y is fp32 either way); W and `a`
        come from the layer."""

        @staticmethod
        def forward(ctx, x, bias, layer):
            M, N = x.shape[0], layer.out_features
            y = torch.empty((M, N), dtype=torch.float32, device=x.device)
            sgemm = layer.plan.sgemm_bf16 if x.dtype == torch.bfloat16 else layer.plan.sgemm
            if layer.a is None:
                sgemm(x, bias, y, M, N, "basic", 0.0, _stream(x.device))
            else:
                sgemm(x, bias, y, M, N, "prelu_basic", layer.a, _stream(x.device))
                ctx.save_for_backward(y)  # the mask is the forward's own predicate on its output
            ctx.layer = layer
            ctx.x_dtype = x.dtype
            return y

        @staticmethod
        def backward(ctx, g):
            layer = ctx.layer
            need_dx, need_db = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
            if not (need_dx or need_db):
                return None, None, None
            if g.dtype != torch.float32 or not g.is_cuda:
                raise TcscError(f"TernaryLinear backward: expected an fp32 CUDA gradient, got {g.dtype} on {g.device}")
            g = g.contiguous()
            M, N, K = g.shape[0], layer.out_features, layer.in_features
            stream = _stream(g.device)
            y = ctx.saved_tensors[0] if layer.a is not None else None
            masked = y is not None and need_dx  # identity activation: dZ is g itself
            dz = torch.empty_like(g) if masked else g
            db = torch.empty(N, dtype=torch.float32, device=g.device) if need_db else None
            if masked or need_db:
                prelu_backward(g, y, layer.a or 0.0, dz if masked else None, db, M, N, stream=stream)
            dx = None
            if need_dx:
                dx = torch.empty((M, K), dtype=torch.float32, device=g.device)
                layer._transposed().sgemm_t(dz, dx, M, K, stream)
                if ctx.x_dtype != torch.float32:  # autograd wants the input's dtype
                    dx = dx.to(ctx.x_dtype)
            return dx, db, None

    class TernaryLinear(torch.nn.Module):
        """``y = act(x . W + bias)`` with a frozen ternary ``W`` (K x N).

        W:    a dense K x N tensor or array with entries in {-1, 0, +1}, or a
              :class:`tcsc_amd.TcscMatrix` (kept by reference; do not free it
              while the layer lives).  W is not a parameter and has no grad.
        bias: N fp32 values (tensor or array) for the ``nn.Parameter``; default zeros.
        a:    the PReLU slope ``act(v) = v < 0 ? a * v : v``, a fixed float as in
              the reference, or None for the identity activation.
        device: the GPU ordinal the plans live on.

        ``forward`` takes fp32 or bf16 CUDA tensors of shape (..., K) on that device
        and returns fp32 (..., N); a bf16 x goes through ``tcsc_gpu_sgemm_bf16`` with
        no fp32 copy, and its gradient (computed in fp32) is returned as bf16.  The transposed plan for ``dX`` is built on the first
        backward that needs it, or by :meth:`reserve`.  One module must not be
        used from several streams at once (the plans own their workspaces).
        """

        def __init__(self, W, bias=None, a: float | None = None, device: int = 0):
            super().__init__()
            self._W = _ternary_matrix(W, "TernaryLinear")
            self.in_features, self.out_features = self._W.rows, self._W.cols
            self.a = None if a is None else float(a)
            self.device_index = int(device)
            dev = torch.device("cuda", self.device_index)
            self.bias = torch.nn.Parameter(_bias_tensor(bias, self.out_features, dev, "TernaryLinear"))
            self.plan = Plan(self._W, 0, self.out_features, self.device_index, _stream(dev))
            self.transposed_plan = None  # built by the first backward that needs dX, or by reserve()
            self._i8_rows, self._i8_xq, self._i8_scale = 0, None, None  # forward_int8's buffers

        def _transposed(self) -> Plan:
            if self.transposed_plan is None:
                dev = torch.device("cuda", self.device_index)
                self.transposed_plan = Plan.transposed(self._W, 0, self.out_features, self.device_index, _stream(dev))
            return self.transposed_plan

        def reserve(self, max_rows: int, int8: bool = False, decode: bool = False) -> None:
            """Workspaces of both plans for up to max_rows rows (the flattened leading
            dimensions), building the transposed plan if it is absent: afterwards a
            forward + backward step allocates nothing in the library and can be captured.
            int8=True also builds the plan's int8 image (``Plan.enable_i8``) and the
            buffers :meth:`forward_int8` quantizes into, for up to max_rows rows.
            decode=True (with int8=True) also builds the 2-bit image (``Plan.enable_w2``):
            :meth:`forward_int8` calls of up to 16 rows then stream it (the decode path)."""
            if decode and not int8:
                raise TcscError("TernaryLinear.reserve: decode=True needs int8=True (the 2-bit image is made from "
                                "the int8 one)")
            self.plan.reserve(max_rows)
            self._transposed().reserve(max_rows)
            if int8:
                self.plan.enable_i8(_stream(torch.device("cuda", self.device_index)))
                self._i8_buffers(max_rows)
            if decode:
                self.plan.enable_w2(_stream(torch.device("cuda", self.device_index)))

        def _i8_buffers(self, rows: int):
            """(Xq, scale) for `rows` rows: kept from the last reserve, grown when a call needs more."""
            if self._i8_rows < rows:
                dev = torch.device("cuda", self.device_index)
                self._i8_xq = torch.empty((rows, self.in_features), dtype=torch.int8, device=dev)
                self._i8_scale = torch.empty(rows, dtype=torch.float32, device=dev)
                self._i8_rows = rows
            return self._i8_xq, self._i8_scale

        def forward_int8(self, x):
            """Inference with int8 activations: ``Plan.sgemm_q8`` quantizes the rows of the fp32 or bf16 x per
            row (the arithmetic of ``tcsc_amd.quantize_rows_i8``; the scales, and off the fused route the int8
            copy, go into buffers the layer keeps) and computes ``act(scale * (q . W) + bias)`` on the current
            stream -- in one launch where the call decodes and fusing pays, as the quantizer followed by
            ``Plan.sgemm_i8`` elsewhere, with the same bits either way.  On the int8 MFMA path after
            ``reserve(rows, int8=True)``; without the image the gather serves the call.  No backward:
            raises when grad is enabled and x requires grad."""
            if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
                raise TcscError("TernaryLinear.forward_int8: x must be an fp32 or bf16 CUDA tensor")
            if torch.is_grad_enabled() and x.requires_grad:
                raise TcscError("TernaryLinear.forward_int8 is inference only: x requires grad")
            if x.device.index != self.device_index or self.bias.device != x.device:
                raise TcscError(f"TernaryLinear: x on {x.device}, bias on {self.bias.device}, plans on cuda:"
                                f"{self.device_index}")
            if x.dim() < 1 or x.shape[-1] != self.in_features:
                raise TcscError(f"TernaryLinear: x has shape {tuple(x.shape)}, expected (..., {self.in_features})")
            lead = x.shape[:-1]
            x2 = x.detach().reshape(-1, self.in_features).contiguous()
            M, K, N = x2.shape[0], self.in_features, self.out_features
            xq, scale = self._i8_buffers(M)
            stream = _stream(x.device)
            y = torch.empty((M, N), dtype=torch.float32, device=x.device)
            if self.a is None:
                self.plan.sgemm_q8(x2, xq, scale, self.bias.detach(), y, M, N, "basic", 0.0, stream)
            else:
                self.plan.sgemm_q8(x2, xq, scale, self.bias.detach(), y, M, N, "prelu_basic", self.a, stream)
            return y.reshape(*lead, N)

        def forward(self, x):
            if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
                raise TcscError("TernaryLinear: x must be an fp32 or bf16 CUDA tensor")
            if x.device.index != self.device_index or self.bias.device != x.device:
                raise TcscError(f"TernaryLinear: x on {x.device}, bias on {self.bias.device}, plans on cuda:"
                                f"{self.device_index}")
            if x.dim() < 1 or x.shape[-1] != self.in_features:
                raise TcscError(f"TernaryLinear: x has shape {tuple(x.shape)}, expected (..., {self.in_features})")
            if self.bias.dtype != torch.float32 or not self.bias.is_contiguous():
                raise TcscError("TernaryLinear: bias must stay a contiguous fp32 tensor")
            lead = x.shape[:-1]
            y = _TernaryLinearFn.apply(x.reshape(-1, self.in_features).contiguous(), self.bias, self)
            return y.reshape(*lead, self.out_features)

        def extra_repr(self) -> str:
            return f"in_features={self.in_features}, out_features={self.out_features}, nnz={self._W.nnz}, a={self.a}"

    class PackedTernaryLinear(torch.nn.Module):
        """Inference-only ``y = act(scale * weight_scale * (q . W) + bias)`` on a packed plan (``Plan.packed``):
        of ``W`` the layer holds the 2-bit image alone, a quarter byte per weight.

        W, bias, a, device: as :class:`TernaryLinear` takes them; the bias is a buffer, not a parameter.
        weight_scale: None, one float (the beta of a per-tensor ternarization, ``tcsc_amd.ternarize_absmean``)
        or N values (one per output column); kept as a buffer of N floats and applied in the kernel's epilogue
        after the row scale and before the bias.  out_dtype: torch.float32 or torch.bfloat16, what ``forward``
        returns -- written by the kernel, rounded to nearest even from the fp32 value (``Plan.sgemm_q8``).
        ``state_dict()`` carries ``weight_scale`` only when the layer has one.
        ``forward`` takes an fp32 or bf16 CUDA tensor of shape (..., K) and calls ``Plan.sgemm_q8``, which
        quantizes its rows to int8 (the arithmetic of ``tcsc_amd.quantize_rows_i8``) and multiplies: up to 16
        rows k_decode8q in one launch where fusing pays, the quantizer and k_decode8 elsewhere, k_gemm8w2
        above -- the bits of ``TernaryLinear.forward_int8`` on the int8 MFMA path.
        norm_weight, norm_eps: with norm_eps given the layer reads ``RMSNorm(x) * norm_weight`` in place of x
        (norm_weight: K values, or None for all ones): ``forward`` calls ``Plan.sgemm_q8_norm``, the norm in the
        library's pinned arithmetic (``tcsc_amd.rmsnorm_rows``) inside the quantizer's launch, or inside the one
        decode launch where fusing pays.  norm_weight is a buffer: ``state_dict()`` carries it when the layer has
        one; norm_eps is a constructor argument, as ``a`` is.  Without norm_eps the layer is what it was.
        ``forward(x, residual=r)`` returns ``r + layer(x)`` from the same launches (``tcsc_gpu_sgemm_q8_res``): r has
        shape (..., N), dtype out_dtype, the layer's device and a unit last stride (contiguous, or two-dimensional
        with a row pitch), and must not require grad.  The add is one fp32 add ahead of the one rounding to
        out_dtype, so a bf16 layer gives ``(fp32 layer(x) + r.float()).to(bfloat16)``, not the twice-rounded
        ``layer(x) + r``.  ``inplace=True`` writes the sum into r and returns r.  A layer with ``a`` set (PReLU)
        refuses a residual.
        decode_rows: None, 16 .. 64 or ``tcsc_amd.DECODE_ROWS_AUTO``: the plan's ``Plan.set_decode_rows`` setting,
        the most rows a forward sends through the one-launch decode kernel after the quantizer (None: the
        library's default, 16).  A runtime setting: the same bits either way, not part of ``state_dict()``, and
        kept across ``load_state_dict``.
        There is no backward and no transposed plan: it raises when grad is enabled and x requires grad.
        """

        def __init__(self, W, bias=None, a: float | None = None, device: int = 0, weight_scale=None,
                     out_dtype=torch.float32, norm_weight=None, norm_eps: float | None = None, decode_rows=None):
            super().__init__()
            Wm = _ternary_matrix(W, "PackedTernaryLinear")  # only read here: the plan keeps no reference to it
            self.in_features, self.out_features, self.nnz = Wm.rows, Wm.cols, Wm.nnz
            self.a = None if a is None else float(a)
            self.device_index = int(device)
            self.out_dtype = _out_dtype(out_dtype)
            dev = torch.device("cuda", self.device_index)
            self.register_buffer("bias", _bias_tensor(bias, self.out_features, dev, "PackedTernaryLinear"))
            self.register_buffer("weight_scale", _weight_scale_tensor(weight_scale, self.out_features, dev))
            nw, self.norm_eps = _norm_args(norm_weight, norm_eps, self.in_features, dev)
            self.register_buffer("norm_weight", nw)
            self.plan = Plan.packed(Wm, 0, self.out_features, self.device_index, _stream(dev))
            self._rows, self._xq, self._scale = 0, None, None
            self.decode_rows = None
            self.set_decode_rows(decode_rows)

        def set_decode_rows(self, decode_rows) -> None:
            """Sets ``decode_rows`` (None keeps the plan as it is) on the plan the layer has, and on every plan a
            ``load_state_dict`` gives it later."""
            self.decode_rows = None if decode_rows is None else int(decode_rows)
            if self.plan is not None and self.decode_rows is not None:
                self.plan.set_decode_rows(self.decode_rows)

        @classmethod
        def from_float(cls, Wf, bias=None, a: float | None = None, device: int = 0, out_dtype=torch.float32,
                       norm_weight=None, norm_eps: float | None = None, decode_rows=None):
            """The layer of a float weight matrix Wf (K x N): ``T, beta = tcsc_amd.ternarize_absmean(Wf)``, then
            the packed plan of T with the per-tensor ``weight_scale = beta``, so that the layer computes
            ``act(x . (beta T) + bias)`` on the quantized x."""
            if torch.is_tensor(Wf):
                Wf = Wf.detach().cpu().numpy()
            T, beta = ternarize_absmean(Wf)
            return cls(T, bias, a, device, weight_scale=float(beta), out_dtype=out_dtype, norm_weight=norm_weight,
                       norm_eps=norm_eps, decode_rows=decode_rows)

        @classmethod
        def empty(cls, in_features: int, out_features: int, a: float | None = None, device: int = 0,
                  out_dtype=torch.float32, norm_eps: float | None = None, decode_rows=None):
            """A layer of this shape with a zero bias, no weight scale and no plan yet: ``load_state_dict`` fills it
            from a ``state_dict()`` of a layer of the same shape (its ``weight_scale`` and ``norm_weight`` included,
            when it has them; a state with a ``norm_weight`` needs a layer made with norm_eps).
            Until then ``forward`` and ``reserve`` raise."""
            self = cls.__new__(cls)
            torch.nn.Module.__init__(self)
            self.in_features, self.out_features, self.nnz = int(in_features), int(out_features), 0
            self.a = None if a is None else float(a)
            self.device_index = int(device)
            self.out_dtype = _out_dtype(out_dtype)
            dev = torch.device("cuda", self.device_index)
            self.register_buffer("bias", torch.zeros(self.out_features, dtype=torch.float32, device=dev))
            self.register_buffer("weight_scale", None)
            _, self.norm_eps = _norm_args(None, norm_eps, self.in_features, dev)
            self.register_buffer("norm_weight", None)
            self.plan = None
            self._rows, self._xq, self._scale = 0, None, None
            self.decode_rows = None if decode_rows is None else int(decode_rows)  # set on the plan a load builds
            return self

        def _loaded_plan(self, what: str) -> Plan:
            if self.plan is None:
                raise TcscError(f"PackedTernaryLinear.{what}: the layer is empty (PackedTernaryLinear.empty): load a "
                                "state_dict first")
            return self.plan

        def _save_to_state_dict(self, destination, prefix, keep_vars):
            """``bias`` (the buffer), ``weight_scale`` (a buffer too, so only when the layer has one: a buffer that
            is None is not saved) and ``w2``: the plan's 2-bit image as a uint8 tensor, a fresh copy made at this
            call -- not a registered buffer, so the layer does not hold the image twice."""
            super()._save_to_state_dict(destination, prefix, keep_vars)
            dev = torch.device("cuda", self.device_index)
            destination[prefix + "w2"] = self._loaded_plan("state_dict").w2_image(_stream(dev))

        def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                  error_msgs):
            """Rebuilds the plan from ``w2`` (``Plan.packed_from_image``, the device path).  ``bias`` and ``w2``
            must be there and the image must have the size of this layer's shape, whatever ``strict`` says:
            TcscError otherwise, with the layer unchanged.  ``weight_scale`` is taken when present (N values) and
            the layer has none afterwards when it is absent.  The plan it replaces is destroyed with its
            workspace, so a ``reserve`` made before the load is gone: reserve again."""
            for key in ("bias", "w2"):
                if prefix + key not in state_dict:
                    raise TcscError(f"PackedTernaryLinear.load_state_dict: missing key {prefix + key!r}")
            w2, bias = state_dict[prefix + "w2"], state_dict[prefix + "bias"]
            if not torch.is_tensor(bias) or bias.numel() != self.out_features:
                raise TcscError(f"PackedTernaryLinear.load_state_dict: {prefix}bias must hold {self.out_features} values")
            want = w2_image_bytes(self.in_features, self.out_features)
            if not torch.is_tensor(w2) or w2.dtype != torch.uint8 or w2.numel() != want:
                got = f"{tuple(w2.shape)} {w2.dtype}" if torch.is_tensor(w2) else type(w2).__name__
                raise TcscError(f"PackedTernaryLinear.load_state_dict: {prefix}w2 is {got}, a {self.in_features} x "
                                f"{self.out_features} layer needs {want} uint8 values")
            dev = torch.device("cuda", self.device_index)
            ws = state_dict.get(prefix + "weight_scale")
            if ws is not None and (not torch.is_tensor(ws) or ws.numel() != self.out_features):
                raise TcscError(f"PackedTernaryLinear.load_state_dict: {prefix}weight_scale must hold "
                                f"{self.out_features} values")
            nw = state_dict.get(prefix + "norm_weight")
            if nw is not None and (not torch.is_tensor(nw) or nw.numel() != self.in_features):
                raise TcscError(f"PackedTernaryLinear.load_state_dict: {prefix}norm_weight must hold "
                                f"{self.in_features} values")
            if nw is not None and self.norm_eps is None:
                raise TcscError(f"PackedTernaryLinear.load_state_dict: {prefix}norm_weight for a layer made without "
                                "norm_eps")
            image = w2.detach().to(dev).contiguous()
            plan = Plan.packed_from_image(image, self.in_features, self.out_features, 0, self.device_index, _stream(dev))
            if getattr(self, "decode_rows", None) is not None:
                plan.set_decode_rows(self.decode_rows)
            # the base class copies into the buffers the layer has: give it one of the state's kind
            self.weight_scale = None if ws is None else torch.empty(self.out_features, dtype=torch.float32, device=dev)
            self.norm_weight = None if nw is None else torch.empty(self.in_features, dtype=torch.float32, device=dev)
            super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                          error_msgs)
            if prefix + "w2" in unexpected_keys:  # the base class knows parameters and buffers only
                unexpected_keys.remove(prefix + "w2")
            old, self.plan = self.plan, plan
            self.nnz = plan.info()["nnz"]
            if old is not None:
                old.destroy()

        def _quant_buffers(self, rows: int):
            if self._rows < rows:
                dev = torch.device("cuda", self.device_index)
                self._xq = torch.empty((rows, self.in_features), dtype=torch.int8, device=dev)
                self._scale = torch.empty(rows, dtype=torch.float32, device=dev)
                self._rows = rows
            return self._xq, self._scale

        def reserve(self, max_rows: int) -> None:
            """The plan's workspace (X8 and the split-K slabs) and the quantization buffers for up to max_rows
            rows: afterwards a forward allocates nothing but its output."""
            self._loaded_plan("reserve").reserve(max_rows)
            self._quant_buffers(max_rows)

        def _residual_2d(self, residual, lead, M: int, x):
            """(pointer holder, pitch) of a residual of shape (*lead, N) as M rows of one pitch."""
            N = self.out_features
            if self.a is not None:
                raise TcscError("PackedTernaryLinear: a layer with a PReLU (a is set) takes no residual")
            if not torch.is_tensor(residual) or residual.dtype != self.out_dtype or residual.device != x.device:
                raise TcscError(f"PackedTernaryLinear: the residual must be a {self.out_dtype} tensor on {x.device}")
            if tuple(residual.shape) != (*lead, N):
                raise TcscError(f"PackedTernaryLinear: the residual has shape {tuple(residual.shape)}, expected "
                                f"{(*lead, N)}")
            if residual.requires_grad:
                raise TcscError("PackedTernaryLinear is inference only: the residual requires grad")
            if residual.is_contiguous():
                return residual, N
            if residual.dim() == 2 and residual.stride(1) == 1 and residual.stride(0) >= N:
                return residual, residual.stride(0)
            raise TcscError("PackedTernaryLinear: the residual must be contiguous, or two-dimensional with a unit "
                            f"last stride and a row pitch of at least {N} (strides {tuple(residual.stride())})")

        def forward(self, x, residual=None, inplace: bool = False):
            plan = self._loaded_plan("forward")
            if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
                raise TcscError("PackedTernaryLinear: x must be an fp32 or bf16 CUDA tensor")
            if torch.is_grad_enabled() and x.requires_grad:
                raise TcscError("PackedTernaryLinear is inference only: x requires grad")
            if x.device.index != self.device_index or self.bias.device != x.device:
                raise TcscError(f"PackedTernaryLinear: x on {x.device}, bias on {self.bias.device}, plan on cuda:"
                                f"{self.device_index}")
            if x.dim() < 1 or x.shape[-1] != self.in_features:
                raise TcscError(f"PackedTernaryLinear: x has shape {tuple(x.shape)}, expected (..., "
                                f"{self.in_features})")
            lead = x.shape[:-1]
            x2 = x.detach().reshape(-1, self.in_features).contiguous()
            M, K, N = x2.shape[0], self.in_features, self.out_features
            xq, scale = self._quant_buffers(M)
            stream = _stream(x.device)
            if residual is not None:
                r, ldr = self._residual_2d(residual, lead, M, x)
                y, ldy = (r, ldr) if inplace else (torch.empty((M, N), dtype=self.out_dtype, device=x.device), N)
                if self.norm_eps is None:
                    plan.sgemm_q8(x2, xq, scale, self.bias, y, M, ldy, "basic", 0.0, stream,
                                  col_scale=self.weight_scale, residual=r, ldr=ldr)
                else:
                    plan.sgemm_q8_norm(x2, xq, scale, self.bias, y, M, ldy, self.norm_weight, self.norm_eps, "basic",
                                       0.0, stream, col_scale=self.weight_scale, residual=r, ldr=ldr)
                return residual if inplace else y.reshape(*lead, N)
            if inplace:
                raise TcscError("PackedTernaryLinear: inplace=True needs a residual to write into")
            y = torch.empty((M, N), dtype=self.out_dtype, device=x.device)
            variant, a = ("basic", 0.0) if self.a is None else ("prelu_basic", self.a)
            if self.norm_eps is None:
                plan.sgemm_q8(x2, xq, scale, self.bias, y, M, N, variant, a, stream, col_scale=self.weight_scale)
            else:
                plan.sgemm_q8_norm(x2, xq, scale, self.bias, y, M, N, self.norm_weight, self.norm_eps, variant, a,
                                   stream, col_scale=self.weight_scale)
            return y.reshape(*lead, N)

        def extra_repr(self) -> str:
            return (f"in_features={self.in_features}, out_features={self.out_features}, nnz={self.nnz}, a={self.a}, "
                    f"weight_scale={self.weight_scale is not None}, out_dtype={self.out_dtype}"
                    + ("" if self.norm_eps is None else f", norm_eps={self.norm_eps}, "
                       f"norm_weight={self.norm_weight is not None}"))

    class PackedTernaryGLU(torch.nn.Module):
        """Inference-only gated pair ``y = act(g) * u`` on two packed plans, with
        ``g = scale * weight_scale_gate * (q . Wg) + bias_gate`` and u the same on Wu: one
        ``tcsc_amd.sgemm_q8_glu`` call -- up to 16 rows a single decode launch that streams both 2-bit images,
        k_gemm8w2 twice on one packed X above, unless ``set_decode_rows`` admits those rows to the decode launch.

        Wg, Wu: K x H each, as :class:`PackedTernaryLinear` takes W.  bias_*, weight_scale_*: as its bias and
        weight_scale, one per half.  act: 'relu2' (``relu(g)**2``) or 'silu'.  norm_weight, norm_eps, out_dtype,
        device: as there.  ``state_dict()`` carries ``w2_gate`` and ``w2_up`` beside the buffers the layer has
        (an absent buffer is None and is not saved); ``empty(K, H).load_state_dict(...)`` and ``reserve(rows)``
        work as in :class:`PackedTernaryLinear`."""

        _HALVES = ("gate", "up")

        def __init__(self, Wg, Wu, bias_gate=None, bias_up=None, weight_scale_gate=None, weight_scale_up=None,
                     act: str = "relu2", norm_weight=None, norm_eps: float | None = None, out_dtype=torch.float32,
                     device: int = 0):
            super().__init__()
            mats = [_ternary_matrix(W, "PackedTernaryGLU") for W in (Wg, Wu)]
            if (mats[0].rows, mats[0].cols) != (mats[1].rows, mats[1].cols):
                raise TcscError(f"PackedTernaryGLU: Wg is {mats[0].rows} x {mats[0].cols}, Wu {mats[1].rows} x "
                                f"{mats[1].cols}")
            self._init_common(mats[0].rows, mats[0].cols, act, norm_eps, out_dtype, device)
            dev = torch.device("cuda", self.device_index)
            self.register_buffer("bias_gate", _bias_tensor(bias_gate, self.out_features, dev, "PackedTernaryGLU"))
            self.register_buffer("bias_up", _bias_tensor(bias_up, self.out_features, dev, "PackedTernaryGLU"))
            self.register_buffer("weight_scale_gate", _weight_scale_tensor(weight_scale_gate, self.out_features, dev))
            self.register_buffer("weight_scale_up", _weight_scale_tensor(weight_scale_up, self.out_features, dev))
            nw, _ = _norm_args(norm_weight, norm_eps, self.in_features, dev)
            self.register_buffer("norm_weight", nw)
            self.plans = [Plan.packed(m, 0, self.out_features, self.device_index, _stream(dev)) for m in mats]

        def _init_common(self, K: int, H: int, act, norm_eps, out_dtype, device):
            from . import GLU_ACT_ID

            if act not in GLU_ACT_ID:
                raise TcscError(f"PackedTernaryGLU: act must be one of {sorted(GLU_ACT_ID)}, got {act!r}")
            self.in_features, self.out_features, self.act = int(K), int(H), act
            self.device_index = int(device)
            self.out_dtype = _out_dtype(out_dtype)
            _, self.norm_eps = _norm_args(None, norm_eps, self.in_features, torch.device("cuda", self.device_index))
            self.plans = None
            self._rows, self._xq, self._scale, self._g = 0, None, None, None
            self.decode_rows = None

        def set_decode_rows(self, rows) -> None:
            """Sets ``Plan.set_decode_rows_multi(rows)`` (16 .. 64 or ``tcsc_amd.DECODE_ROWS_AUTO``; None keeps the
            plans as they are) on both plans, and on those a later ``load_state_dict`` builds: a forward of 17 ..
            rows rows is then the one gated decode launch, the same bits."""
            self.decode_rows = None if rows is None else int(rows)
            if self.plans is not None and self.decode_rows is not None:
                for plan in self.plans:
                    plan.set_decode_rows_multi(self.decode_rows)

        @classmethod
        def from_float(cls, Wg, Wu, bias_gate=None, bias_up=None, act: str = "relu2", norm_weight=None,
                       norm_eps: float | None = None, out_dtype=torch.float32, device: int = 0):
            """The layer of two float matrices (K x H each): each ternarized by ``tcsc_amd.ternarize_absmean``, its
            beta the half's per-tensor weight scale."""
            tb = [ternarize_absmean(W.detach().cpu().numpy() if torch.is_tensor(W) else W) for W in (Wg, Wu)]
            return cls(tb[0][0], tb[1][0], bias_gate, bias_up, float(tb[0][1]), float(tb[1][1]), act, norm_weight,
                       norm_eps, out_dtype, device)

        @classmethod
        def empty(cls, in_features: int, out_features: int, act: str = "relu2", norm_eps: float | None = None,
                  out_dtype=torch.float32, device: int = 0):
            """A layer of this shape with zero biases, no weight scales and no plans yet, for ``load_state_dict``."""
            self = cls.__new__(cls)
            torch.nn.Module.__init__(self)
            self._init_common(in_features, out_features, act, norm_eps, out_dtype, device)
            dev = torch.device("cuda", self.device_index)
            for h in cls._HALVES:
                self.register_buffer("bias_" + h, torch.zeros(self.out_features, dtype=torch.float32, device=dev))
                self.register_buffer("weight_scale_" + h, None)
            self.register_buffer("norm_weight", None)
            return self

        def _loaded_plans(self, what: str):
            if self.plans is None:
                raise TcscError(f"PackedTernaryGLU.{what}: the layer is empty (PackedTernaryGLU.empty): load a "
                                "state_dict first")
            return self.plans

        def _save_to_state_dict(self, destination, prefix, keep_vars):
            super()._save_to_state_dict(destination, prefix, keep_vars)
            st = _stream(torch.device("cuda", self.device_index))
            for h, plan in zip(self._HALVES, self._loaded_plans("state_dict")):
                destination[prefix + "w2_" + h] = plan.w2_image(st)

        def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                  error_msgs):
            """Rebuilds both plans from ``w2_gate`` and ``w2_up``; they and the two biases must be there, whatever
            ``strict`` says (TcscError otherwise, the layer unchanged); the weight scales and ``norm_weight`` are
            taken when present and the layer has none afterwards when absent."""
            who, K, H = "PackedTernaryGLU.load_state_dict", self.in_features, self.out_features
            dev = torch.device("cuda", self.device_index)
            want = w2_image_bytes(K, H)
            for h in self._HALVES:
                for key in ("bias_" + h, "w2_" + h):
                    if prefix + key not in state_dict:
                        raise TcscError(f"{who}: missing key {prefix + key!r}")
                b, w2 = state_dict[prefix + "bias_" + h], state_dict[prefix + "w2_" + h]
                if not torch.is_tensor(b) or b.numel() != H:
                    raise TcscError(f"{who}: {prefix}bias_{h} must hold {H} values")
                if not torch.is_tensor(w2) or w2.dtype != torch.uint8 or w2.numel() != want:
                    raise TcscError(f"{who}: {prefix}w2_{h} must hold the {want} uint8 values of a {K} x {H} image")
                ws = state_dict.get(prefix + "weight_scale_" + h)
                if ws is not None and (not torch.is_tensor(ws) or ws.numel() != H):
                    raise TcscError(f"{who}: {prefix}weight_scale_{h} must hold {H} values")
            nw = state_dict.get(prefix + "norm_weight")
            if nw is not None and (not torch.is_tensor(nw) or nw.numel() != K or self.norm_eps is None):
                raise TcscError(f"{who}: {prefix}norm_weight must hold {K} values, on a layer made with norm_eps")
            plans = [Plan.packed_from_image(state_dict[prefix + "w2_" + h].detach().to(dev).contiguous(), K, H, 0,
                                            self.device_index, _stream(dev)) for h in self._HALVES]
            for h in self._HALVES:  # the base class copies into the buffers the layer has: one of the state's kind
                has = state_dict.get(prefix + "weight_scale_" + h) is not None
                setattr(self, "weight_scale_" + h, torch.empty(H, dtype=torch.float32, device=dev) if has else None)
            self.norm_weight = None if nw is None else torch.empty(K, dtype=torch.float32, device=dev)
            super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                          error_msgs)
            for h in self._HALVES:
                if prefix + "w2_" + h in unexpected_keys:
                    unexpected_keys.remove(prefix + "w2_" + h)
            if getattr(self, "decode_rows", None) is not None:
                for p in plans:
                    p.set_decode_rows_multi(self.decode_rows)
            old, self.plans = self.plans, plans
            for p in old or ():
                p.destroy()

        def _scratch(self, rows: int):
            if self._rows < rows:
                dev = torch.device("cuda", self.device_index)
                self._xq = torch.empty((rows, self.in_features), dtype=torch.int8, device=dev)
                self._scale = torch.empty(rows, dtype=torch.float32, device=dev)
                # the gate values of the MFMA route (more than 16 rows); the decode launch needs none
                self._g = torch.empty((rows, self.out_features), dtype=torch.float32, device=dev) if rows > 16 else None
                self._rows = rows
            return self._xq, self._scale, self._g

        def reserve(self, max_rows: int) -> None:
            """The gate plan's workspace and the layer's scratch (the quantized X, the row scales and, above 16
            rows, the gate values) for up to max_rows rows: afterwards a forward allocates nothing but its output."""
            self._loaded_plans("reserve")[0].reserve(max_rows)
            self._scratch(max_rows)

        def forward(self, x):
            from . import sgemm_q8_glu

            gate, up = self._loaded_plans("forward")
            if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
                raise TcscError("PackedTernaryGLU: x must be an fp32 or bf16 CUDA tensor")
            if torch.is_grad_enabled() and x.requires_grad:
                raise TcscError("PackedTernaryGLU is inference only: x requires grad")
            if x.device.index != self.device_index or x.dim() < 1 or x.shape[-1] != self.in_features:
                raise TcscError(f"PackedTernaryGLU: x has shape {tuple(x.shape)} on {x.device}, expected (..., "
                                f"{self.in_features}) on cuda:{self.device_index}")
            lead = x.shape[:-1]
            x2 = x.detach().reshape(-1, self.in_features).contiguous()
            M, H = x2.shape[0], self.out_features
            xq, scale, g = self._scratch(M)
            y = torch.empty((M, H), dtype=self.out_dtype, device=x.device)
            sgemm_q8_glu(gate, up, x2, xq, scale, self.bias_gate, self.bias_up, y, M, H, self.act,
                         self.weight_scale_gate, self.weight_scale_up, self.norm_weight, self.norm_eps, g,
                         _stream(x.device))
            return y.reshape(*lead, H)

        def extra_repr(self) -> str:
            return (f"in_features={self.in_features}, out_features={self.out_features}, act={self.act}, "
                    f"out_dtype={self.out_dtype}" + ("" if self.norm_eps is None else f", norm_eps={self.norm_eps}"))

    class PackedTernaryMLP(torch.nn.Module):
        """The two-call FFN of a BitNet-style block: ``down(subnorm(act(gate(norm(x))) * up(norm(x))))`` as a
        :class:`PackedTernaryGLU` with a bf16 output (``glu``) and a :class:`PackedTernaryLinear` with its own
        RMSNorm in front (``down``: K = the hidden width).  Both are built by the caller; ``reserve`` and the
        state dict are the two layers'.  ``forward(x, residual=r, inplace=...)`` passes the residual to ``down``
        (:class:`PackedTernaryLinear`): the FFN with its skip connection in two library calls.
        decode_rows, if given, is set on ``down`` alone (``PackedTernaryLinear.set_decode_rows``): the gated call
        has a setting of its own, ``glu.set_decode_rows``."""

        def __init__(self, glu: PackedTernaryGLU, down: PackedTernaryLinear, decode_rows=None):
            super().__init__()
            if down.in_features != glu.out_features:
                raise TcscError(f"PackedTernaryMLP: the GLU gives {glu.out_features} columns, down takes "
                                f"{down.in_features}")
            self.glu, self.down = glu, down
            if decode_rows is not None:
                down.set_decode_rows(decode_rows)

        def reserve(self, max_rows: int) -> None:
            self.glu.reserve(max_rows)
            self.down.reserve(max_rows)

        def forward(self, x, residual=None, inplace: bool = False):
            return self.down(self.glu(x), residual=residual, inplace=inplace)

    class PackedTernaryGroup(torch.nn.Module):
        """Inference-only group of 1 to 4 ternary matrices on one input, the Q, K and V
        projections of an attention block for instance: ``y_i = scale * weight_scale_i * (q . W_i) + bias_i`` for
        every member in one ``tcsc_amd.sgemm_q8_group`` call -- up to 16 rows a single decode launch over all
        the 2-bit images, one packed X and one k_gemm8w2 per member above (unless ``set_decode_rows`` admits those rows
        to the decode launch).  Each y_i has the bits of a
        :class:`PackedTernaryLinear` (a None) built from the same inputs.

        Ws: the matrices, K x N_i each, as :class:`PackedTernaryLinear` takes W; the N_i are free.  biases,
        weight_scales: None, or one entry per member (each as that layer's bias / weight_scale).  norm_weight,
        norm_eps, out_dtype, device: shared, as there.  ``forward(x)`` writes one ``[rows, sum N_i]`` tensor and
        returns the members' column slices of it as a tuple (views of one allocation: ``torch.cat`` is free).
        ``state_dict()`` carries ``w2_<i>`` beside ``bias_<i>`` and, where the member has one,
        ``weight_scale_<i>``; ``empty(K, [N_i]).load_state_dict(...)`` and ``reserve(rows)`` work as in
        :class:`PackedTernaryLinear`."""

        def __init__(self, Ws, biases=None, weight_scales=None, norm_weight=None, norm_eps: float | None = None,
                     out_dtype=torch.float32, device: int = 0):
            super().__init__()
            from . import GROUP_MAX

            Ws = list(Ws)
            if not 1 <= len(Ws) <= GROUP_MAX:
                raise TcscError(f"PackedTernaryGroup: {len(Ws)} matrices, a group holds 1 to {GROUP_MAX}")
            mats = [_ternary_matrix(W, "PackedTernaryGroup") for W in Ws]
            if any(m.rows != mats[0].rows for m in mats):
                raise TcscError(f"PackedTernaryGroup: the matrices have {[m.rows for m in mats]} rows, one K is needed")
            biases = [None] * len(mats) if biases is None else list(biases)
            weight_scales = [None] * len(mats) if weight_scales is None else list(weight_scales)
            if len(biases) != len(mats) or len(weight_scales) != len(mats):
                raise TcscError("PackedTernaryGroup: biases and weight_scales take one entry per matrix")
            self._init_common(mats[0].rows, [m.cols for m in mats], norm_eps, out_dtype, device)
            dev = torch.device("cuda", self.device_index)
            for k, n in enumerate(self.out_features_list):
                self.register_buffer(f"bias_{k}", _bias_tensor(biases[k], n, dev, "PackedTernaryGroup"))
                self.register_buffer(f"weight_scale_{k}", _weight_scale_tensor(weight_scales[k], n, dev))
            nw, _ = _norm_args(norm_weight, norm_eps, self.in_features, dev)
            self.register_buffer("norm_weight", nw)
            self.plans = [Plan.packed(m, 0, m.cols, self.device_index, _stream(dev)) for m in mats]

        def _init_common(self, K: int, cols, norm_eps, out_dtype, device):
            from . import GROUP_MAX

            cols = [int(n) for n in cols]
            if not 1 <= len(cols) <= GROUP_MAX:
                raise TcscError(f"PackedTernaryGroup: {len(cols)} members, a group holds 1 to {GROUP_MAX}")
            self.in_features, self.out_features_list = int(K), cols
            self.out_features = sum(cols)
            self.device_index = int(device)
            self.out_dtype = _out_dtype(out_dtype)
            _, self.norm_eps = _norm_args(None, norm_eps, self.in_features, torch.device("cuda", self.device_index))
            self.plans = None
            self._rows, self._xq, self._scale = 0, None, None
            self.decode_rows = None

        def set_decode_rows(self, rows) -> None:
            """Sets ``Plan.set_decode_rows_multi(rows)`` (16 .. 64 or ``tcsc_amd.DECODE_ROWS_AUTO``; None keeps the
            plans as they are) on every member's plan, and on those a later ``load_state_dict`` builds: a forward of 17 ..
            rows rows is then the one grouped decode launch, the same bits."""
            self.decode_rows = None if rows is None else int(rows)
            if self.plans is not None and self.decode_rows is not None:
                for plan in self.plans:
                    plan.set_decode_rows_multi(self.decode_rows)

        @classmethod
        def from_float(cls, Wfs, biases=None, norm_weight=None, norm_eps: float | None = None,
                       out_dtype=torch.float32, device: int = 0):
            """The layer of float matrices (K x N_i): each ternarized by ``tcsc_amd.ternarize_absmean``, its beta the
            member's per-tensor weight scale."""
            tb = [ternarize_absmean(W.detach().cpu().numpy() if torch.is_tensor(W) else W) for W in Wfs]
            return cls([t for t, _ in tb], biases, [float(b) for _, b in tb], norm_weight, norm_eps, out_dtype, device)

        @classmethod
        def empty(cls, in_features: int, out_features_list, norm_eps: float | None = None, out_dtype=torch.float32,
                  device: int = 0):
            """A layer of these shapes with zero biases, no weight scales and no plans yet, for ``load_state_dict``."""
            self = cls.__new__(cls)
            torch.nn.Module.__init__(self)
            self._init_common(in_features, out_features_list, norm_eps, out_dtype, device)
            dev = torch.device("cuda", self.device_index)
            for k, n in enumerate(self.out_features_list):
                self.register_buffer(f"bias_{k}", torch.zeros(n, dtype=torch.float32, device=dev))
                self.register_buffer(f"weight_scale_{k}", None)
            self.register_buffer("norm_weight", None)
            return self

        def _loaded_plans(self, what: str):
            if self.plans is None:
                raise TcscError(f"PackedTernaryGroup.{what}: the layer is empty (PackedTernaryGroup.empty): load a "
                                "state_dict first")
            return self.plans

        def _save_to_state_dict(self, destination, prefix, keep_vars):
            super()._save_to_state_dict(destination, prefix, keep_vars)
            st = _stream(torch.device("cuda", self.device_index))
            for k, plan in enumerate(self._loaded_plans("state_dict")):
                destination[f"{prefix}w2_{k}"] = plan.w2_image(st)

        def _load_from_state_dict(self, state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                  error_msgs):
            """Rebuilds every plan from its ``w2_<i>``; the images and the biases must be there, whatever
            ``strict`` says (TcscError otherwise, the layer unchanged); the weight scales and ``norm_weight`` are
            taken when present and the layer has none afterwards when absent."""
            who, K = "PackedTernaryGroup.load_state_dict", self.in_features
            dev = torch.device("cuda", self.device_index)
            for k, n in enumerate(self.out_features_list):
                for key in (f"bias_{k}", f"w2_{k}"):
                    if prefix + key not in state_dict:
                        raise TcscError(f"{who}: missing key {prefix + key!r}")
                b, w2 = state_dict[f"{prefix}bias_{k}"], state_dict[f"{prefix}w2_{k}"]
                want = w2_image_bytes(K, n)
                if not torch.is_tensor(b) or b.numel() != n:
                    raise TcscError(f"{who}: {prefix}bias_{k} must hold {n} values")
                if not torch.is_tensor(w2) or w2.dtype != torch.uint8 or w2.numel() != want:
                    raise TcscError(f"{who}: {prefix}w2_{k} must hold the {want} uint8 values of a {K} x {n} image")
                ws = state_dict.get(f"{prefix}weight_scale_{k}")
                if ws is not None and (not torch.is_tensor(ws) or ws.numel() != n):
                    raise TcscError(f"{who}: {prefix}weight_scale_{k} must hold {n} values")
            nw = state_dict.get(prefix + "norm_weight")
            if nw is not None and (not torch.is_tensor(nw) or nw.numel() != K or self.norm_eps is None):
                raise TcscError(f"{who}: {prefix}norm_weight must hold {K} values, on a layer made with norm_eps")
            plans = [Plan.packed_from_image(state_dict[f"{prefix}w2_{k}"].detach().to(dev).contiguous(), K, n, 0,
                                            self.device_index, _stream(dev))
                     for k, n in enumerate(self.out_features_list)]
            for k, n in enumerate(self.out_features_list):  # the base class copies into the buffers the layer has
                has = state_dict.get(f"{prefix}weight_scale_{k}") is not None
                setattr(self, f"weight_scale_{k}", torch.empty(n, dtype=torch.float32, device=dev) if has else None)
            self.norm_weight = None if nw is None else torch.empty(K, dtype=torch.float32, device=dev)
            super()._load_from_state_dict(state_dict, prefix, local_metadata, strict, missing_keys, unexpected_keys,
                                          error_msgs)
            for k in range(len(self.out_features_list)):
                if f"{prefix}w2_{k}" in unexpected_keys:
                    unexpected_keys.remove(f"{prefix}w2_{k}")
            if getattr(self, "decode_rows", None) is not None:
                for p in plans:
                    p.set_decode_rows_multi(self.decode_rows)
            old, self.plans = self.plans, plans
            for p in old or ():
                p.destroy()

        def _scratch(self, rows: int):
            if self._rows < rows:
                dev = torch.device("cuda", self.device_index)
                self._xq = torch.empty((rows, self.in_features), dtype=torch.int8, device=dev)
                self._scale = torch.empty(rows, dtype=torch.float32, device=dev)
                self._rows = rows
            return self._xq, self._scale

        def reserve(self, max_rows: int) -> None:
            """Every member plan's workspace and the layer's scratch (the quantized X and the row scales) for up
            to max_rows rows: afterwards a forward allocates nothing but its output."""
            for plan in self._loaded_plans("reserve"):
                plan.reserve(max_rows)
            self._scratch(max_rows)

        def forward(self, x):
            from . import sgemm_q8_group

            plans = self._loaded_plans("forward")
            if not torch.is_tensor(x) or x.dtype not in (torch.float32, torch.bfloat16) or not x.is_cuda:
                raise TcscError("PackedTernaryGroup: x must be an fp32 or bf16 CUDA tensor")
            if torch.is_grad_enabled() and x.requires_grad:
                raise TcscError("PackedTernaryGroup is inference only: x requires grad")
            if x.device.index != self.device_index or x.dim() < 1 or x.shape[-1] != self.in_features:
                raise TcscError(f"PackedTernaryGroup: x has shape {tuple(x.shape)} on {x.device}, expected (..., "
                                f"{self.in_features}) on cuda:{self.device_index}")
            lead = x.shape[:-1]
            x2 = x.detach().reshape(-1, self.in_features).contiguous()
            M, n = x2.shape[0], len(plans)
            xq, scale = self._scratch(M)
            y = torch.empty((M, self.out_features), dtype=self.out_dtype, device=x.device)
            ys = list(torch.split(y, self.out_features_list, dim=1))
            sgemm_q8_group(plans, x2, xq, scale, [getattr(self, f"bias_{k}") for k in range(n)], ys, M,
                           [self.out_features] * n, [getattr(self, f"weight_scale_{k}") for k in range(n)],
                           self.norm_weight, self.norm_eps, _stream(x.device))
            # the leading dimensions of x back on the row axis: views still (a reshape of a column slice would copy)
            return tuple(v.unflatten(0, tuple(lead)) if lead else v[0] for v in ys)

        def extra_repr(self) -> str:
            return (f"in_features={self.in_features}, out_features={self.out_features_list}, "
                    f"out_dtype={self.out_dtype}" + ("" if self.norm_eps is None else f", norm_eps={self.norm_eps}"))

    return {"TernaryLinear": TernaryLinear, "PackedTernaryLinear": PackedTernaryLinear,
            "PackedTernaryGLU": PackedTernaryGLU, "PackedTernaryMLP": PackedTernaryMLP,
            "PackedTernaryGroup": PackedTernaryGroup}


def __getattr__(name):
    global _classes
    if name in __all__:
        if _classes is None:
            _classes = _define()
        return _classes[name]
    raise AttributeError(f"module {__name__!r} has no attribute {name!r}")
