"""Incremental (key/value-cached) decoding of the prior's decoder stack.

The reference re-runs the full decoder over all positions for every sampled
token (sample.py:268-283): O(S^2) layer passes per codemap.  Decoder
self-attention is causal (priors/transformer.py:483-500) and inputs at positions
< p never change once written, so row p of a full pass equals the row computed
from cached keys / values of rows <= p; the encoder memory and its projected
keys / values are computed once.  `tests/test_prior_gpu.py` checks that the
incremental rows equal the full-sequence pass."""
from __future__ import annotations

from typing import List

import torch

from . import _ops


def kv_cache_format(kv_cache_dtype) -> int:
    """`isi_prior_state.kv_format` of a cache dtype: float32 (the default) or bfloat16 (opt-in: half the bytes the cached
    attention streams per position, keys / values rounded to 8 significand bits).  Anything else: ValueError."""
    if kv_cache_dtype is torch.float32:
        return 0
    if kv_cache_dtype is torch.bfloat16:
        return 1
    raise ValueError(f"kv_cache_dtype must be torch.float32 or torch.bfloat16, not {kv_cache_dtype!r}")


def _is_aligned(layers) -> bool:
    from VQCPCB.transformer.transformer_custom import TransformerAlignedDecoderLayerCustom
    return any(isinstance(l, TransformerAlignedDecoderLayerCustom) for l in layers)


def _refuse_aligned(layers) -> None:
    """The key/value-cached loops attend over ALL memory rows; the aligned decoder layer restricts them per target event."""
    if _is_aligned(layers):
        raise NotImplementedError("KV-cached sampling is not built for use_aligned_decoder=True (full passes work)")


def _single_source_check(model, layers, S_t: int, S_src: int, device) -> bool:
    """True when every decoder row attends ONE source row, j = p // Cd: an aligned decoder (source events of one token) or the
    identity memory mask.  Raises ValueError where the full forward fails for the geometry, NotImplementedError for source
    events of more than one token (Ce > 1)."""
    aligned, identity = _is_aligned(layers), bool(getattr(model, "use_identity_memory_mask", False))
    if not (aligned or identity):
        return False
    if model.source_num_channels != 1:
        raise NotImplementedError("single-source cross-attention needs one source token per event (Ce == 1)")
    if aligned:
        layers[0].alignment_mask(S_t, S_src, device)        # ValueError: a target event without a source event
    if identity:
        if S_t != S_src:
            raise ValueError(f"identity memory mask: {S_t} target rows against {S_src} source rows")
        if model.target_num_channels != 1:
            raise NotImplementedError("identity memory mask with more than one target token per event")
    return True


class IncrementalDecoder:
    def __init__(self, model, memory: torch.Tensor, batch_size: int, kv_cache_dtype: torch.dtype = torch.float32):
        """memory: [S_src, B, d] encoder output.  kv_cache_dtype: float32, or bfloat16 for 16-bit caches."""
        kv_cache_format(kv_cache_dtype)
        self.kv_cache_dtype = kv_cache_dtype
        dec = model.transformer.decoder
        self.layers = list(dec.layers)
        _refuse_aligned(self.layers)
        if getattr(model, "use_identity_memory_mask", False):
            raise NotImplementedError("incremental decoding attends over every memory row: not built for "
                                      "use_identity_memory_mask=True (NativeSampler is)")
        self.model = model
        d = model.d_model
        S_t = model.target_transformer_sequence_length_with_start_symbol
        self.B, self.d = batch_size, d
        self.Cd, self.Ed = model.target_num_channels, model.target_num_events_with_start_symbol
        self.Ce, self.Ee = model.source_num_channels, model.source_num_events_with_start_symbol
        memory = memory.contiguous()
        self.S_src = memory.shape[0]
        # (a 16-bit cache: torch's copy rounds to nearest-even)
        self.memory_kv: List[torch.Tensor] = [l.multihead_attn.project_kv(memory).to(kv_cache_dtype) for l in self.layers]
        self.cache: List[torch.Tensor] = [
            torch.zeros(S_t, batch_size, 2 * d, dtype=kv_cache_dtype, device=memory.device) for _ in self.layers]
        if batch_size > 32:
            raise NotImplementedError("incremental decoding supports batch sizes up to 32 (NativeSampler: 256)")

    def _linear(self, x, weight, bias, relu=False, residual=None, out=None):
        """Row GEMV of up to 8 rows per launch (`isi_linear_rows_f32`); larger batches go in groups of 8 rows -- a row's
        result does not depend on the rows it shares a launch with."""
        M = x.shape[0]
        if M <= 8:
            return _ops.linear_rows(x, weight, bias, relu=relu, residual=residual, out=out)
        if out is None:
            out = torch.empty(M, weight.shape[0], dtype=torch.float32, device=x.device)
        for lo in range(0, M, 8):
            hi = min(M, lo + 8)
            _ops.linear_rows(x[lo:hi], weight, bias, relu=relu, residual=residual[lo:hi] if residual is not None else None,
                             out=out[lo:hi])
        return out

    @torch.no_grad()
    def step(self, p: int, x: torch.Tensor) -> torch.Tensor:
        """Decoder output row at sequence position p for the input row x [B, d]."""
        d = self.d
        for l, layer in enumerate(self.layers):
            sa, ca = layer.self_attn, layer.multihead_attn
            W, b = sa.in_proj_weight, sa.in_proj_bias
            q = self._linear(x, W[:d], b[:d])
            if self.kv_cache_dtype is torch.float32:
                self._linear(x, W[d:], b[d:], out=self.cache[l][p])       # k|v of this row -> cache slot p
            else:
                self.cache[l][p].copy_(self._linear(x, W[d:], b[d:]))     # ... rounded to the cache's format
            kc = self.cache[l]
            a = _ops.rel_attention_decode(q, kc[..., :d], kc[..., d:], sa.rel_embeddings, sa.nhead,
                                          n_keys=p + 1, q_pos=p, Cq=self.Cd, Ck=self.Cd, Ek=self.Ed)
            x1 = layer.norm1.run(self._linear(a, sa.out_proj.weight, sa.out_proj.bias, residual=x))
            Wc, bc = ca.in_proj_weight, ca.in_proj_bias
            qc = self._linear(x1, Wc[:d], bc[:d])
            mkv = self.memory_kv[l]
            c = _ops.rel_attention_decode(qc, mkv[..., :d], mkv[..., d:], ca.rel_embeddings, ca.nhead,
                                          n_keys=self.S_src, q_pos=p, Cq=self.Cd, Ck=self.Ce, Ek=self.Ee)
            x2 = layer.norm2.run(self._linear(c, ca.out_proj.weight, ca.out_proj.bias, residual=x1))
            h = self._linear(x2, layer.linear1.weight, layer.linear1.bias, relu=True)
            x = layer.norm3.run(self._linear(h, layer.linear2.weight, layer.linear2.bias, residual=x2))
        return x

    @torch.no_grad()
    def logits(self, out_row: torch.Tensor) -> torch.Tensor:
        head = self.model.project_transformer_outputs_to_logits
        return self._linear(out_row, head.weight, head.bias)


class NativeSampler:
    """The whole sampling loop in one native call (`isi_prior_sample_run`): all
    per-position launches are enqueued without returning to Python and without
    host synchronisation; sampled indices stay on the device."""

    def __init__(self, model, memory: torch.Tensor, x_seq: torch.Tensor, codes: torch.Tensor,
                 mask_seq, uniforms: torch.Tensor, kv_cache_dtype: torch.dtype = torch.float32,
                 shared_memory: bool = False, log_probs: bool = False, code_bias: torch.Tensor = None,
                 code_bias_index: torch.Tensor = None):
        """shared_memory: the B rows of x_seq are variations of ONE request -- memory is [S_src, 1, d], its projected keys /
        values (or the single-source table) are formed once at batch 1 and every row reads them
        (`isi_prior_state.memory_shared`).
        log_probs: the loop also stores the model's log-probability of every token it commits
        (`isi_prior_state.token_log_probs`) into `self.log_probs` [B, S] float32, zero where nothing was sampled.
        code_bias / code_bias_index: a float32 table [R, n_class] of logit bias rows (-inf bans a class) and an integer
        index [S] or [1, S] (every row) or [B, S], in sequence order, of the table row each token is drawn with; -1: none
        (`isi_prior_code_bias`, passed beside the state to `isi_prior_sample_run_bias`).  The sampler keeps both alive; their contents are read when the loop runs."""
        import ctypes as C
        kv_format = kv_cache_format(kv_cache_dtype)        # before anything is allocated
        self.kv_cache_dtype = kv_cache_dtype
        self.shared_memory = bool(shared_memory)
        if self.shared_memory and memory.shape[1] != 1:
            raise ValueError(f"shared_memory: memory is [S_src, 1, d], not {tuple(memory.shape)}")
        import numpy as np
        from .. import _hip
        from .transformer import Seq2SeqInputKind
        self._C, self._hip = C, _hip
        dec_layers = list(model.transformer.decoder.layers)
        self.single_source = _single_source_check(model, dec_layers, x_seq.shape[0], memory.shape[0], memory.device)
        if len(dec_layers) > _hip.ISI_MAX_LAYERS:
            raise NotImplementedError(f"more than {_hip.ISI_MAX_LAYERS} decoder layers")
        dev = memory.device
        d, B = model.d_model, x_seq.shape[1]
        if B > 256:
            raise NotImplementedError("native sampling supports batch sizes up to 256")
        self.model = model
        self.keep = []
        w = _hip.isi_prior_w()
        w.d_model, w.nhead = d, model.conditional_model_nhead
        w.dim_feedforward = dec_layers[0].linear1.out_features
        w.n_layers, w.n_class = len(dec_layers), model.n_class_target
        w.Cd, w.Ed = model.target_num_channels, model.target_num_events_with_start_symbol
        w.Ce, w.Ee = model.source_num_channels, model.source_num_events_with_start_symbol

        def ptr(t):
            t = t.detach()
            if not t.is_contiguous():
                t = t.contiguous()
            self.keep.append(t)
            return t.data_ptr()

        def attn(m):
            a = _hip.isi_attn_w()
            a.in_proj_weight, a.in_proj_bias = ptr(m.in_proj_weight), ptr(m.in_proj_bias)
            a.out_proj_weight, a.out_proj_bias = ptr(m.out_proj.weight), ptr(m.out_proj.bias)
            if m.rel_embeddings is not None:
                a.rel_embeddings, a.rel_rows = ptr(m.rel_embeddings), m.rel_embeddings.shape[1]
            return a

        for i, layer in enumerate(dec_layers):
            L = w.layers[i]
            L.self_attn, L.cross_attn = attn(layer.self_attn), attn(layer.multihead_attn)
            L.linear1_w, L.linear1_b = ptr(layer.linear1.weight), ptr(layer.linear1.bias)
            L.linear2_w, L.linear2_b = ptr(layer.linear2.weight), ptr(layer.linear2.bias)
            for k in (1, 2, 3):
                norm = getattr(layer, f"norm{k}")
                setattr(L, f"norm{k}_w", ptr(norm.weight))
                setattr(L, f"norm{k}_b", ptr(norm.bias))
        head = model.project_transformer_outputs_to_logits
        w.logits_w, w.logits_b = ptr(head.weight), ptr(head.bias)
        table = model._embedding_table(Seq2SeqInputKind.Target)
        w.embed_table, w.eff_dim = ptr(table), table.shape[1]
        self.w = w

        memory = memory.contiguous()
        self.memory_kv = self.cross_out = None
        if self.single_source:
            # every row attends one source row: a layer's cross-attention block is a row of out_proj(V(memory)), formed here
            # by the full pass's own two products (the values of its k|v projection, then the out-projection)
            self.cross_out = torch.stack([l.multihead_attn.out_proj.run(l.multihead_attn.project_kv(memory)[..., d:].contiguous())
                                          for l in dec_layers]).contiguous()
        else:
            # (a 16-bit cache: layer by layer through torch's copy, round-to-nearest-even)
            self.memory_kv = torch.stack([l.multihead_attn.project_kv(memory).to(kv_cache_dtype) for l in dec_layers]).contiguous()
        S_t = x_seq.shape[0]
        self.kv_cache = torch.zeros(len(dec_layers), S_t, B, 2 * d, dtype=kv_cache_dtype, device=dev)
        self.x_seq, self.codes = x_seq, codes
        self.mask_host = np.ascontiguousarray(np.asarray(mask_seq, dtype=np.uint8))
        self.uniforms = uniforms.to(device=dev, dtype=torch.float32).contiguous()
        n_scratch = _hip.lib().isi_prior_decode_scratch_floats(C.byref(w), B)
        self.scratch = torch.empty(n_scratch, dtype=torch.float32, device=dev)
        st = _hip.isi_prior_state()
        st.x_seq, st.kv_cache = x_seq.data_ptr(), self.kv_cache.data_ptr()
        if self.single_source:
            st.cross_out = self.cross_out.data_ptr()
        else:
            st.memory_kv = self.memory_kv.data_ptr()
        st.codes, st.mask = codes.data_ptr(), self.mask_host.ctypes.data
        st.uniforms, st.scratch, st.scratch_floats = self.uniforms.data_ptr(), self.scratch.data_ptr(), n_scratch
        st.S_t, st.S_src, st.S, st.B = S_t, memory.shape[0], codes.shape[1], B
        st.start_len = model.target_start_symbol.shape[1]
        st.kv_format = kv_format
        if self.shared_memory:
            st.memory_shared = 1
        self.log_probs = None
        if log_probs:
            self.log_probs = torch.zeros(B, codes.shape[1], dtype=torch.float32, device=dev)
            st.token_log_probs = self.log_probs.data_ptr()
        self.code_bias = self.code_bias_index = self.bias = None
        if (code_bias is None) != (code_bias_index is None):
            raise ValueError("code_bias and code_bias_index go together")
        if code_bias is not None:
            S = codes.shape[1]
            if code_bias.dim() != 2 or code_bias.shape[1] != w.n_class or code_bias.shape[0] < 1:
                raise ValueError(f"code_bias {tuple(code_bias.shape)}: expected [R, {w.n_class}]")
            index = code_bias_index.reshape(1, -1) if code_bias_index.dim() == 1 else code_bias_index
            if index.dim() != 2 or index.shape[1] != S or index.shape[0] not in (1, B):
                raise ValueError(f"code_bias_index {tuple(code_bias_index.shape)}: expected [{S}], [1, {S}] or [{B}, {S}]")
            self.code_bias = code_bias.detach().to(device=dev, dtype=torch.float32).contiguous()
            self.code_bias_index = index.to(device=dev, dtype=torch.int32).contiguous()
            cb = _hip.isi_prior_code_bias()
            cb.code_bias, cb.code_bias_index = self.code_bias.data_ptr(), self.code_bias_index.data_ptr()
            cb.code_bias_count, cb.code_bias_batch = self.code_bias.shape[0], self.code_bias_index.shape[0]
            self.bias = cb
        self.state = st

    @torch.no_grad()
    def prefill(self, p0: int) -> None:
        """Key / value cache rows [0, p0) of every decoder layer from ONE causal pass over those rows (the
        full-sequence GEMM / attention kernels) instead of p0 single-row steps: what an unmasked prefix of an
        inpainting request needs -- its codes are known, only its keys and values are read later."""
        if p0 <= 0:
            return
        from VQCPCB.transformer.transformer_custom import _add_norm
        d = self.model.d_model
        # a shared memory: the rows are identical up to the first sampled position -- the pass runs on row 0 alone and its
        # keys / values are broadcast into the B slots of the cache (one copy)
        x = self.x_seq[:p0, :1].contiguous() if self.shared_memory else self.x_seq[:p0].contiguous()
        if self.single_source:
            src_row = torch.arange(p0, device=x.device) // self.model.target_num_channels
        for l, layer in enumerate(self.model.transformer.decoder.layers):
            sa = layer.self_attn
            qkv = sa._project(x, 0)                                  # [p0, B, 3d]
            self.kv_cache[l, :p0] = qkv[..., d:]                     # (a 16-bit cache: torch's copy, round-to-nearest-even)
            kv = qkv[..., d:]
            if self.kv_cache_dtype is not torch.float32:
                kv = self.kv_cache[l, :p0, :x.shape[1]].float()      # the pass attends what the later single steps will read
            a = _ops.rel_attention(qkv[..., :d], kv[..., :d], kv[..., d:], sa.rel_embeddings, sa.nhead,
                                   sa.Cq, sa.Ck, sa.Ek, mask_mode=1)
            x1 = _add_norm(layer, sa.out_proj, a, x, layer.norm1)
            if self.single_source:
                x2 = layer.norm2.run(self.cross_out[l].index_select(0, src_row), residual=x1)   # the loop's table rows
            else:
                # (the batched pass attends with fp32 operands: a 16-bit memory_kv is widened, exactly)
                c = layer.multihead_attn(x1, None, None, kv=self.memory_kv[l].float())
                x2 = _add_norm(layer, layer.multihead_attn.out_proj, c, x1, layer.norm2)
            h = layer.linear1.run(x2, relu=True)
            x = _add_norm(layer, layer.linear2, h, x2, layer.norm3)

    @torch.no_grad()
    def run(self, p_begin: int, p_end: int, temperature: float, top_k: int, top_p: float) -> None:
        C, _hip = self._C, self._hip
        if self.bias is not None:          # (without one: the entry and the launches it always took)
            rc = _hip.lib().isi_prior_sample_run_bias(C.byref(self.w), C.byref(self.state), C.byref(self.bias), p_begin, p_end,
                                                      float(temperature), int(top_k), float(top_p),
                                                      C.c_void_p(_hip.stream_ptr(self.x_seq.device)))
            _hip.check(rc, "isi_prior_sample_run_bias")
            return
        rc = _hip.lib().isi_prior_sample_run(C.byref(self.w), C.byref(self.state), p_begin, p_end,
                                             float(temperature), int(top_k), float(top_p),
                                             C.c_void_p(_hip.stream_ptr(self.x_seq.device)))
        _hip.check(rc, "isi_prior_sample_run")

    def plan_rows(self, pos, commit, temperature=None, top_k=None, top_p=None) -> int:
        """A ragged plan (`isi_prior_sample_run_rows`): pos / commit [n_steps, B] host arrays -- row b stands at decoder
        position pos[t, b] in step t and draws its token there where commit[t, b]; optional per-row temperature / top-k /
        top-p tensors [B].  Returns the number of steps."""
        import numpy as np
        C, _hip = self._C, self._hip
        dev = self.x_seq.device
        self.pos_host = np.ascontiguousarray(np.asarray(pos, dtype=np.int32))
        self.commit_host = np.ascontiguousarray(np.asarray(commit, dtype=np.uint8))
        if self.pos_host.ndim != 2 or self.pos_host.shape != self.commit_host.shape or self.pos_host.shape[1] != self.state.B:
            raise ValueError(f"ragged plan: pos {self.pos_host.shape} / commit {self.commit_host.shape} for a batch of "
                             f"{self.state.B}")
        self.pos_dev = torch.from_numpy(self.pos_host).to(dev)
        self.commit_dev = torch.from_numpy(self.commit_host).to(dev)
        r = _hip.isi_prior_rows()
        r.pos, r.commit = self.pos_dev.data_ptr(), self.commit_dev.data_ptr()
        r.pos_host, r.commit_host = self.pos_host.ctypes.data, self.commit_host.ctypes.data
        self.row_params = []
        for name, value, dtype in (("temperature", temperature, torch.float32), ("top_k", top_k, torch.int32),
                                   ("top_p", top_p, torch.float32)):
            if value is not None:
                t = torch.as_tensor(value).to(device=dev, dtype=dtype).reshape(-1).contiguous()
                self.row_params.append(t)
                setattr(r, name, t.data_ptr())
        r.n_steps = self.pos_host.shape[0]
        self.rows = r
        return r.n_steps

    @torch.no_grad()
    def run_rows(self, t_begin: int, t_end: int, temperature: float, top_k: int, top_p: float) -> None:
        """Steps [t_begin, t_end) of the plan set by `plan_rows`; the scalars stand for rows without per-row values."""
        C, _hip = self._C, self._hip
        if self.bias is not None:
            rc = _hip.lib().isi_prior_sample_run_rows_bias(C.byref(self.w), C.byref(self.state), C.byref(self.rows),
                                                           C.byref(self.bias), t_begin, t_end, float(temperature), int(top_k),
                                                           float(top_p), C.c_void_p(_hip.stream_ptr(self.x_seq.device)))
            _hip.check(rc, "isi_prior_sample_run_rows_bias")
            return
        rc = _hip.lib().isi_prior_sample_run_rows(C.byref(self.w), C.byref(self.state), C.byref(self.rows), t_begin, t_end,
                                                  float(temperature), int(top_k), float(top_p),
                                                  C.c_void_p(_hip.stream_ptr(self.x_seq.device)))
        _hip.check(rc, "isi_prior_sample_run_rows")
