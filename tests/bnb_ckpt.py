"""Test-side writer of pre-quantized bitsandbytes 4-bit NF4 checkpoints (bitsandbytes is not installed): functional.quantize_4bit restated
(blockwise absmax over the flattened weight, nearest NF4 code, element 2i in the high nibble), double quantisation of the block scales
(offset = mean, 8-bit codes of a 256-entry signed map per nested block of 256), and QuantState.as_dict(packed=True)'s key layout."""
import json
import os

import torch

from vibevoice_rocm_amd.weights import NF4_TABLE, _nf4_thresholds, fp8_matrix_names

# a signed, non-uniform 256-entry map standing in for bnb's dynamic map (the loader uses whatever map the file stores)
_t = torch.linspace(-1.0, 1.0, 256, dtype=torch.float64)
DYN_MAP = (_t * _t.abs()).float()


def quantize_flat(w: torch.Tensor, blocksize: int):
    """(codes uint8 [numel], absmax fp32 [ceil(numel / blocksize)]) of the flattened weight, bnb's blockwise NF4."""
    flat = w.detach().float().reshape(-1)
    nb = -(-flat.numel() // blocksize)
    x = torch.zeros(nb * blocksize)
    x[: flat.numel()] = flat
    x = x.view(nb, blocksize)
    absmax = x.abs().amax(dim=1)
    zero = absmax == 0
    inv = torch.where(zero, torch.zeros_like(absmax), torch.reciprocal(absmax))
    codes = torch.searchsorted(_nf4_thresholds(), (x * inv[:, None]).contiguous(), right=False).to(torch.uint8)
    codes = torch.where(zero[:, None], torch.full_like(codes, 7), codes)
    return codes.reshape(-1)[: flat.numel()].contiguous(), absmax.contiguous()


def pack_codes(codes: torch.Tensor) -> torch.Tensor:
    """uint8 [ceil(n / 2)]: element 2i in the high nibble, 2i + 1 in the low one (an odd count leaves the last low nibble 0)."""
    c = codes.reshape(-1).to(torch.uint8)
    if c.numel() % 2:
        c = torch.cat([c, torch.zeros(1, dtype=torch.uint8)])
    return ((c[0::2] << 4) | c[1::2]).contiguous()


def double_quant(absmax: torch.Tensor, nested_blocksize: int = 256):
    """(uint8 codes [nblocks], nested_absmax fp32 [ceil(nblocks / nested_blocksize)], offset float)."""
    offset = float(absmax.mean())
    a = absmax - torch.tensor(offset, dtype=torch.float32)
    nb = -(-a.numel() // nested_blocksize)
    x = torch.zeros(nb * nested_blocksize)
    x[: a.numel()] = a
    x = x.view(nb, nested_blocksize)
    nabs = x.abs().amax(dim=1).clamp_min(1e-30)
    y = (x / nabs[:, None]).reshape(-1)[: a.numel()]
    codes = torch.searchsorted((DYN_MAP[1:] + DYN_MAP[:-1]) / 2, y.contiguous()).to(torch.uint8)     # nearest map entry
    return codes, nabs.contiguous(), offset


def quant_state_tensor(state: dict) -> torch.Tensor:
    return torch.frombuffer(bytearray(json.dumps(state).encode("utf-8")), dtype=torch.uint8).clone()


def bnb_tensors(name: str, w: torch.Tensor = None, blocksize: int = 64, double: bool = False, codes: torch.Tensor = None,
                absmax: torch.Tensor = None, shape=None, dtype: str = "float16"):
    """The safetensors entries of one quantised matrix `name` (".weight" key).  Either w (quantised here) or codes + absmax as given
    (flattened order) with `shape`."""
    if codes is None:
        shape = tuple(w.shape)
        codes, absmax = quantize_flat(w, blocksize)
    packed = pack_codes(codes)
    state = {"quant_type": "nf4", "blocksize": blocksize, "dtype": dtype, "shape": list(shape)}
    out = {name: packed.view(-1, 1), name + ".quant_map": torch.tensor(NF4_TABLE, dtype=torch.float32)}
    if double:
        q, nabs, off = double_quant(absmax.reshape(-1).float())
        state.update(nested_blocksize=256, nested_dtype="float32", nested_offset=off)
        out.update({name + ".absmax": q, name + ".nested_absmax": nabs, name + ".nested_quant_map": DYN_MAP.clone()})
    else:
        out[name + ".absmax"] = absmax.reshape(-1).float().contiguous()
    out[name + ".quant_state.bitsandbytes__nf4"] = quant_state_tensor(state)
    return out


def linear_names(cfg, sd, which: str):
    """'all': every nn.Linear weight (2-D, not the embedding / lm_head: HF's modules_to_not_convert); 'companion': fp8_matrix_names."""
    if which == "companion":
        return [n for n in fp8_matrix_names(cfg) if n in sd]
    return [k for k, v in sd.items() if k.endswith(".weight") and v.dim() == 2 and "embed_tokens" not in k and k != "lm_head.weight"]


def write_bnb_dir(path, cfg, sd, which="all", blocksize=64, double=False, rest_dtype=None, given=None):
    """A pre-quantized checkpoint directory of `sd`: the `which` matrices in bnb NF4 form (given: {name: (codes [N, K], absmax)} taken as
    they are, blocksize 64 over rows), every other tensor plain (cast to rest_dtype when given, floating tensors only), config.json with the
    quantization_config block transformers writes.  Returns the names written in 4-bit form."""
    from vibevoice_rocm_amd.modeling import save_checkpoint_dir
    names = linear_names(cfg, sd, which) if given is None else list(given)
    out = {}
    for k, v in sd.items():
        if k in names:
            continue
        v = v.detach().cpu()
        out[k] = v.to(rest_dtype) if rest_dtype is not None and v.is_floating_point() else v
    for n in names:
        if given is not None:
            c, a = given[n]
            out.update(bnb_tensors(n, codes=c.reshape(-1).cpu(), absmax=a.reshape(-1).cpu(), shape=tuple(c.shape), blocksize=64))
        else:
            out.update(bnb_tensors(n, sd[n].cpu(), blocksize=blocksize, double=double))
    save_checkpoint_dir(str(path), cfg, out)
    cj = os.path.join(str(path), "config.json")
    with open(cj) as f:
        j = json.load(f)
    j["quantization_config"] = {"quant_method": "bitsandbytes", "load_in_4bit": True, "load_in_8bit": False, "bnb_4bit_quant_type": "nf4",
                                "bnb_4bit_use_double_quant": bool(double), "bnb_4bit_compute_dtype": "float16",
                                "bnb_4bit_quant_storage": "uint8", "llm_int8_skip_modules": ["lm_head"]}
    with open(cj, "w") as f:
        json.dump(j, f, indent=2, sort_keys=True)
    return names
