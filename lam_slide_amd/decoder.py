"""Frozen stage-1 decode on the MI355X: ``first_stage.decode(latents, entities)`` of the reference
(models/composites/lightning_base.py:42-44 = ``Decoder(post_quant(latents), entities)``, models/components/decoder.py:12-102),
the step right after the sampler.  Inference only, fp32, through ``lsl_decode`` of liblamslide_hip.so.  The peptide
variant ``DecoderQuerySplitter`` (decoder.py:313-411) is recognised by its ``decoder.extender.1.*`` parameters.

The weights are taken from the first-stage state dict under the reference's own names (``post_quant.1.*``, ``decoder.*``); the
constructor arguments that cannot be read off the weight shapes carry the reference's names (decoder.py:14-29).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Optional, Sequence

import torch
from torch import Tensor

from . import _lib

_ACT = {"gelu_erf": 1, "gelu": 1, "gelu_tanh": 2}
MAX_HEADS = 8  # LSL_DECODE_MAX_HEADS: the heads of one lsl_decode_heads call


def renorm_table(table: Tensor, max_norm: Optional[float]) -> Tensor:
    """nn.Embedding(max_norm=...) rescales every looked-up row whose L2 norm exceeds max_norm, in place, at forward time
    (entity_embeddings.py:25; torch embedding_renorm_: scale = max_norm / (norm + 1e-7)).  Applied to the whole table once."""
    if max_norm is None:
        return table.clone()
    norms = table.norm(dim=-1, keepdim=True)
    return torch.where(norms > max_norm, table * (max_norm / (norms + 1e-7)), table)


class _Stage1:
    """What Stage1Decoder and Stage1Encoder share: the float32 weights ``_sd`` (and ``qk_norm``), their device copies behind the native
    handle, and the scratch of a call - one buffer per (device, stream), so two calls of one object on two streams never write the same
    LayerNorm, q/k/v and attention buffers.  A subclass names the library's ``_create`` / ``_destroy`` symbols and builds the
    description and the weight struct in ``_describe(dev)``."""
    _create = _destroy = ""

    def _init_handle(self, device) -> None:
        self._handle = C.c_void_p()
        self._dev_tensors: List[Tensor] = []
        self._scratch = _lib.Scratch()
        self._head_ptrs = None
        if device is not None:
            self.to(device)

    def _p(self, key: str, dev) -> Optional[int]:
        if key not in self._sd:
            return None
        t = self._sd[key].to(dev).contiguous()
        self._dev_tensors.append(t)
        return t.data_ptr()

    def _block(self, prefix: str, dev, cross: bool) -> "_lib.DecBlock":
        g = lambda name: self._p(f"{prefix}.{name}", dev)  # noqa: E731
        return _lib.DecBlock(
            ln_w=g("attn.norm.weight"), ln_b=g("attn.norm.bias"),
            lnc_w=g("attn.norm_context.weight") if cross else None, lnc_b=g("attn.norm_context.bias") if cross else None,
            w_q=g("attn.fn.to_q.weight") if cross else g("attn.fn.to_qkv.weight"), w_kv=g("attn.fn.to_kv.weight") if cross else None,
            w_out=g("attn.fn.to_out.weight"), b_out=g("attn.fn.to_out.bias"),
            q_scale=g("attn.fn.norm.query_norm.scale") if self.qk_norm else None, k_scale=g("attn.fn.norm.key_norm.scale") if self.qk_norm else None,
            ff_ln_w=g("ff.norm.weight"), ff_ln_b=g("ff.norm.bias"), ff_w1=g("ff.fn.net.0.0.weight"), ff_b1=g("ff.fn.net.0.0.bias"),
            ff_w2=g("ff.fn.net.1.weight"), ff_b2=g("ff.fn.net.1.bias"))

    def _blocks(self, prefix: str, n: int, dev, cross: bool):
        return (_lib.DecBlock * max(n, 1))(*[self._block(f"{prefix}.{i}", dev, cross) for i in range(n)])

    def _destroy_handle(self) -> None:
        if self._handle:
            getattr(_lib.load(), self._destroy)(self._handle)
            self._handle = C.c_void_p()

    def to(self, device):
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} runs on the MI355X only (no CPU path)")
        self._destroy_handle()
        self._dev_tensors = []
        self._head_ptrs = None  # (Stage1Decoder.decode_heads: the device copies of every head, made on first use)
        desc, w = self._describe(dev)
        _lib.check(getattr(_lib.load(), self._create)(C.byref(desc), C.byref(w), C.byref(self._handle)))
        self.device = dev
        return self

    def __del__(self):
        try:
            self._destroy_handle()
        except Exception:
            pass

    def _on(self, x: Tensor, method: str) -> None:
        """The handle on x's device, before a call."""
        if not x.is_cuda:
            raise RuntimeError(f"{type(self).__name__}.{method} needs CUDA/HIP tensors (no CPU path)")
        if not self._handle or self.device != x.device:
            self.to(x.device)


class Stage1Decoder(_Stage1):
    _create, _destroy = "lsl_decoder_create", "lsl_decoder_destroy"

    def __init__(self, state_dict: Dict[str, Tensor], *, num_head_latent: int, dim_head_latent: int, num_head_cross: int,
                 dim_head_cross: int, act: str = "gelu_erf", output: str = "pos", max_norm: Optional[float] = 1.0,
                 device: Optional[torch.device] = None):
        if act not in _ACT:
            raise ValueError(f"unknown activation {act!r} (gelu_erf | gelu_tanh)")
        sd = {k.replace("_orig_mod.", ""): v for k, v in state_dict.items()}
        need = ["post_quant.1.weight", "post_quant.1.bias", "decoder.entity_embedding.embedding.weight", "decoder.query_mlp.1.weight",
                f"decoder.output_layers.{output}.0.weight", f"decoder.output_layers.{output}.2.weight"]
        for k in need:
            if k not in sd:
                raise KeyError(k)
        self.num_block_attn = len({k.split(".")[2] for k in sd if k.startswith("decoder.self_attn_blocks.")})
        self.num_block_cross = len({k.split(".")[2] for k in sd if k.startswith("decoder.cross_attn_blocks.")})
        self.qk_norm = "decoder.output_block.attn.fn.norm.query_norm.scale" in sd
        self.dim_latent, self.in_dim = sd["post_quant.1.weight"].shape
        self.n_entities, self.dim_emb = sd["decoder.entity_embedding.embedding.weight"].shape
        self.dim_query = sd["decoder.query_mlp.1.weight"].shape[0]
        self.out_dim = sd[f"decoder.output_layers.{output}.2.weight"].shape[0]
        self.heads_latent, self.dim_head_latent = int(num_head_latent), int(dim_head_latent)
        self.heads_cross, self.dim_head_cross = int(num_head_cross), int(dim_head_cross)
        inner_c = self.heads_cross * self.dim_head_cross
        if tuple(sd["decoder.output_block.attn.fn.to_q.weight"].shape) != (inner_c, self.dim_query):
            raise ValueError("num_head_cross * dim_head_cross does not match decoder.output_block.attn.fn.to_q.weight")
        if self.num_block_attn and sd["decoder.self_attn_blocks.0.attn.fn.to_qkv.weight"].shape[0] != 3 * self.heads_latent * self.dim_head_latent:
            raise ValueError("num_head_latent * dim_head_latent does not match decoder.self_attn_blocks.0.attn.fn.to_qkv.weight")
        self.act, self.output, self.max_norm = act, output, max_norm
        # every head of decoder.output_layers in the state dict's (= the ModuleDict's) order: name -> out_dim (decode_heads)
        self.heads: Dict[str, int] = {}
        for k in sd:
            if k.startswith("decoder.output_layers.") and k.endswith(".2.weight"):
                self.heads[k[len("decoder.output_layers."):-len(".2.weight")]] = int(sd[k].shape[0])
        self._sd = {k: v.detach().to(torch.float32) for k, v in sd.items() if k.startswith(("post_quant.", "decoder."))}
        # DecoderQuerySplitter (decoder.py:384-388): Conv1d(D, D*N, 1) then "B (D N) L -> B (L N) D"; as a Linear whose rows are
        # reordered from channel d*N + n to n*D + d, the output of one latent IS its N context tokens back to back
        self.num_split = 0
        if "decoder.extender.1.weight" in self._sd:
            w, b = self._sd.pop("decoder.extender.1.weight")[..., 0], self._sd.pop("decoder.extender.1.bias")
            n = w.shape[0] // self.dim_latent
            self.num_split = int(n)
            self._sd["decoder.extender.rows"] = w.reshape(self.dim_latent, n, self.dim_latent).permute(1, 0, 2).reshape(n * self.dim_latent, self.dim_latent).contiguous()
            self._sd["decoder.extender.rows_bias"] = b.reshape(self.dim_latent, n).t().reshape(-1).contiguous()
        self._sd["decoder.entity_embedding.embedding.weight"] = renorm_table(self._sd["decoder.entity_embedding.embedding.weight"], max_norm)
        self._init_handle(device)

    def _describe(self, dev):
        w = _lib.DecoderWeights(
            pq_w=self._p("post_quant.1.weight", dev), pq_b=self._p("post_quant.1.bias", dev),
            table=self._p("decoder.entity_embedding.embedding.weight", dev),
            qm_w=self._p("decoder.query_mlp.1.weight", dev), qm_b=self._p("decoder.query_mlp.1.bias", dev),
            self_blocks=self._blocks("decoder.self_attn_blocks", self.num_block_attn, dev, False),
            cross_blocks=self._blocks("decoder.cross_attn_blocks", self.num_block_cross, dev, True), out_block=self._block("decoder.output_block", dev, True),
            ext_w=self._p("decoder.extender.rows", dev), ext_b=self._p("decoder.extender.rows_bias", dev),
            head_w1=self._p(f"decoder.output_layers.{self.output}.0.weight", dev), head_b1=self._p(f"decoder.output_layers.{self.output}.0.bias", dev),
            head_w2=self._p(f"decoder.output_layers.{self.output}.2.weight", dev), head_b2=self._p(f"decoder.output_layers.{self.output}.2.bias", dev))
        desc = _lib.DecoderDesc(self.in_dim, self.dim_latent, self.dim_query, self.dim_emb, self.n_entities, self.heads_latent, self.dim_head_latent,
                                self.heads_cross, self.dim_head_cross, self.num_block_attn, self.num_block_cross, _ACT[self.act], self.out_dim, self.num_split)
        return desc, w

    # -- decode ----------------------------------------------------------------------------------------------
    @torch.no_grad()
    def decode(self, latents: Tensor, entities: Tensor) -> Tensor:
        """latents [F, L, C] fp32, entities [F, A] integer -> [F, A, out_dim] (the reference returns ``{"pos": ...}``;
        this is the tensor of the one head selected by ``output``)."""
        self._on(latents, "decode")
        if latents.dim() != 3 or latents.shape[-1] != self.in_dim or entities.dim() != 2 or entities.shape[0] != latents.shape[0]:
            raise ValueError("expected latents [F, L, C] and entities [F, A]")
        F_, L, _ = latents.shape
        A = entities.shape[1]
        z = latents.contiguous().float()
        ent = entities.contiguous().to(torch.int64)
        ws = self._scratch.get(z.device, _lib.load().lsl_decode_workspace_bytes(self._handle, F_, L, A))
        out = torch.empty(F_, A, self.out_dim, dtype=torch.float32, device=z.device)
        _lib.call(z.device, "lsl_decode", self._handle, z.data_ptr(), ent.data_ptr(), F_, L, A, out.data_ptr(), ws.data_ptr(), ws.numel())
        return out

    __call__ = decode

    @torch.no_grad()
    def decode_heads(self, latents: Tensor, entities: Tensor, outputs: Optional[Sequence[str]] = None) -> Dict[str, Tensor]:
        """What the reference's ``Decoder.forward`` returns (decoder.py:97-102): ``{name: [F, A, out_dim]}`` for every head of
        ``decoder.output_layers`` in the state dict's order, or for the named ``outputs`` in the order given - the trunk once and the heads
        on its rows, one ``lsl_decode_heads`` call.  Each tensor has the bits of ``Stage1Decoder(output=name).decode``."""
        self._on(latents, "decode_heads")
        if latents.dim() != 3 or latents.shape[-1] != self.in_dim or entities.dim() != 2 or entities.shape[0] != latents.shape[0]:
            raise ValueError("expected latents [F, L, C] and entities [F, A]")
        names = list(self.heads) if outputs is None else list(outputs)
        for n in names:
            if n not in self.heads:
                raise KeyError(f"decoder.output_layers.{n}")
        if not 1 <= len(names) <= MAX_HEADS or len(set(names)) != len(names):
            raise ValueError(f"expected 1..{MAX_HEADS} distinct heads, got {names}")
        F_, L, _ = latents.shape
        A = entities.shape[1]
        z = latents.contiguous().float()
        ent = entities.contiguous().to(torch.int64)
        dev = z.device
        if self._head_ptrs is None:
            self._head_ptrs = {n: tuple(self._p(f"decoder.output_layers.{n}.{i}.{wb}", dev) for i, wb in ((0, "weight"), (0, "bias"), (2, "weight"), (2, "bias")))
                               for n in self.heads}
        heads = (_lib.DecoderHead * len(names))(*[_lib.DecoderHead(*self._head_ptrs[n], self.heads[n]) for n in names])
        outs = {n: torch.empty(F_, A, self.heads[n], dtype=torch.float32, device=dev) for n in names}
        ptrs = (C.c_void_p * len(names))(*[outs[n].data_ptr() for n in names])
        ws = self._scratch.get(dev, _lib.load().lsl_decode_workspace_bytes(self._handle, F_, L, A))
        _lib.call(dev, "lsl_decode_heads", self._handle, heads, len(names), z.data_ptr(), ent.data_ptr(), F_, L, A, ptrs, ws.data_ptr(), ws.numel())
        return outs
