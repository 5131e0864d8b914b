"""Pre-quantized bitsandbytes NF4 checkpoints on the MI355X: vv_nf4_import bit for bit against the host restatement (bf16 matrix and VV_NF4
companion), a checkpoint of quantize_nf4's own codes giving exactly the weight_quant="nf4" model, the reference fork's 4-bit from_pretrained call
against the oracle on the checkpoint's effective weights, and the loaded companions holding the file's codes and scales unchanged."""
import pytest
import torch

from bnb_ckpt import bnb_tensors, write_bnb_dir
from conftest import rel_rms

pytestmark = pytest.mark.gpu

REF_QC = dict(load_in_4bit=True, bnb_4bit_quant_type="nf4", bnb_4bit_use_double_quant=True, bnb_4bit_compute_dtype=torch.float16)


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def _rec(name, n, k, bs, double, seed):
    from vibevoice_rocm_amd import bnb
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(n, k, generator=g) / k ** 0.5
    if k >= 128 and n > 1:
        w[1, :64] = 0.0                                            # an all-zero block (code 7, scale 0) when it lies inside a row
    _, recs = bnb.split_prequantized(bnb_tensors(name, w, blocksize=bs, double=double))
    return recs[name]


def _check_import(parts, companion):
    from vibevoice_rocm_amd import bnb
    from vibevoice_rocm_amd.weights import unpack_nf4
    w, cq, cs = bnb.import_nf4(parts, "cuda:0", companion=companion)
    torch.cuda.synchronize()
    want = torch.cat([bnb.dequantize(p) for p in parts], dim=0)
    assert w.dtype == torch.bfloat16 and torch.equal(w.float().cpu(), want), "bf16 matrix differs from the host restatement"
    if not companion:
        assert cq is None and cs is None
        return
    n, k = want.shape
    codes, absmax = unpack_nf4(cq.cpu(), cs.cpu(), n, k)
    want_c = torch.cat([bnb.codes(p).view(p.n, p.k) for p in parts], dim=0)
    want_a = torch.cat([bnb.block_absmax(p).repeat_interleave(p.blocksize // 64).view(p.n, p.k // 64) for p in parts], dim=0)
    assert torch.equal(codes, want_c), "companion codes differ from the file's"
    assert torch.equal(absmax, want_a), "companion scales differ from the file's decoded absmax"
    nq, ku = (n + 3) // 4, (k + 511) // 512                          # padding rows / k: code 0, scale 0
    full_c = torch.stack([cq.cpu() & 15, cq.cpu() >> 4], -1).view(nq, ku, 64, 4, 8).permute(0, 3, 1, 2, 4).reshape(nq * 4, ku * 512)
    assert int(full_c[n:].sum()) == 0 and int(full_c[:, k:].sum()) == 0
    full_a = cs.cpu().view(nq, ku, 4, 8).permute(0, 2, 1, 3).reshape(nq * 4, ku * 8)
    assert float(full_a[n:].abs().sum()) == 0 and float(full_a[:, k // 64:].abs().sum()) == 0


@pytest.mark.parametrize("double", [False, True])
@pytest.mark.parametrize("n,k,bs", [(64, 512, 64), (48, 1024, 128), (40, 1536, 256), (20, 640, 64), (32, 512, 32), (24, 96, 64), (7, 9, 64),
                                    (5, 100, 128), (18944, 3584, 64), (3584, 18944, 64)])
def test_import_bit_exact(n, k, bs, double):
    """vv_nf4_import against bnb.dequantize / codes / block_absmax: blocksize 64 / 128 / 256 (companion) and 32 (none), K = 96 and 100 (blocks
    straddling rows), odd N*K (7 x 9: the last byte half used, a partial last block), the 7B MLP shapes; with and without double quantisation."""
    _need_gpu()
    r = _rec("m.weight", n, k, bs, double, n * 7 + k + bs)
    _check_import([r], r.companion_exact())


@pytest.mark.parametrize("double", [False, True])
def test_import_row_offsets_fused_qkv(double):
    """q, k and v as three calls into one fused destination at row offsets (rows 6 + 5 + 3: groups of 4 rows split across calls)."""
    _need_gpu()
    parts = [_rec(f"{c}.weight", n, 512, 64, double, i) for i, (c, n) in enumerate((("q", 6), ("k", 5), ("v", 3)))]
    _check_import(parts, True)
    parts = [_rec(f"{c}.weight", n, 1536, 128, double, 10 + i) for i, (c, n) in enumerate((("q", 512), ("k", 128), ("v", 128)))]
    _check_import(parts, True)
    _check_import(parts, False)


def test_import_rejections():
    """A companion the layout cannot hold exactly, and bad row ranges, are errors."""
    _need_gpu()
    import ctypes as C

    from vibevoice_rocm_amd import _lib as L
    lib = L.load()
    r = _rec("m.weight", 8, 512, 32, False, 1).to("cuda:0")
    w = torch.empty(8, 512, dtype=torch.bfloat16, device="cuda:0")
    cq, cs = torch.zeros(2 * 1024, dtype=torch.uint8, device="cuda:0"), torch.zeros(2 * 32, device="cuda:0")
    s = L.Nf4Src()
    s.packed, s.absmax, s.quant_map, s.n, s.k, s.blocksize = r.weight.data_ptr(), r.absmax.data_ptr(), r.quant_map.data_ptr(), 8, 512, 32
    assert lib.vv_nf4_import(C.byref(s), w.data_ptr(), 512, 0, 8, cq.data_ptr(), cs.data_ptr(), None) != 0      # blocksize 32
    assert lib.vv_nf4_import(C.byref(s), w.data_ptr(), 512, 1, 8, None, None, None) != 0                        # rows past the destination
    assert lib.vv_nf4_import(C.byref(s), w.data_ptr(), 256, 0, 8, None, None, None) != 0                        # ldw < k
    assert lib.vv_nf4_import(C.byref(s), w.data_ptr(), 512, 0, 8, cq.data_ptr(), None, None) != 0               # half a companion
    assert lib.vv_nf4_import(C.byref(s), w.data_ptr(), 512, 0, 8, None, None, None) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------------------
# whole model at mid shapes
# ---------------------------------------------------------------------------------------------------------------
class _Tok:
    def __init__(self, st, se, sd, eos):
        self.speech_start_id, self.speech_end_id, self.speech_diffusion_id, self.eos_token_id = st, se, sd, eos
        self.bos_token_id = None
        self.pad_id = 0


@pytest.fixture(scope="module")
def mid():
    _need_gpu()
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict
    cfg = VVConfig.preset("mid")
    sd = {k: torch.from_numpy(v) for k, v in synth_state_dict(cfg, 4321).items()}
    return cfg, sd


def _special(cfg):
    V = cfg.vocab
    return V - 4, V - 3, V - 2, V - 1


def _gen(m, cfg, ids, forced, noise, steps=10):
    m.set_ddpm_inference_steps(steps)
    return m.generate(input_ids=ids[None], tokenizer=_Tok(*_special(cfg)), cfg_scale=2.0, forced_tokens=forced, noise=noise)


@pytest.mark.parametrize("graphs", [False, True])
def test_prequantized_of_quantize_nf4_equals_nf4_mode(mid, tmp_path, graphs):
    """A checkpoint holding quantize_nf4's own codes and fp32 absmax (blocksize 64, no double quantisation, companion set only, the rest as
    it is): from_pretrained gives generate() output equal, bit for bit, to weight_quant="nf4" built from the same state dict."""
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    from vibevoice_rocm_amd.weights import fp8_matrix_names, quantize_nf4
    cfg, sd = mid
    given = {}
    for n in fp8_matrix_names(cfg):
        if sd[n].shape[1] % 64 == 0:
            c, a, _ = quantize_nf4(sd[n].to("cuda:0", torch.bfloat16))   # on the device, as the nf4 engine quantises
            given[n] = (c.cpu(), a.cpu())
    write_bnb_dir(tmp_path, cfg, sd, given=given)
    m = M.from_pretrained(str(tmp_path), use_graphs=graphs)
    assert m.weight_quant == "nf4" and m.dtype == torch.bfloat16
    m2 = M(cfg, sd, device="cuda:0", torch_dtype=torch.bfloat16, weight_quant="nf4", use_graphs=graphs)
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, cfg.vocab - 8, (40,), generator=g)
    forced = [ST] + [D] * 4 + [E, ST, D, D, E, EOS]
    noise = torch.randn(6, cfg.latent, generator=g)
    a, b = _gen(m, cfg, ids, forced, noise), _gen(m2, cfg, ids, forced, noise)
    assert a.sequences[0, 40:].tolist() == forced
    assert torch.equal(a.speech_outputs[0].cpu(), b.speech_outputs[0].cpu()), "pre-quantized load != weight_quant='nf4'"


@pytest.fixture(scope="module")
def fork_model(mid, tmp_path_factory):
    """The reference fork's 4-bit branch: every Linear in bnb NF4 (double quantisation), the rest fp16, under <repo>/4bit, loaded with
    config=VibeVoiceConfig.from_pretrained(<bf16 dir>) and quantization_config=BitsAndBytesConfig(...)."""
    from vibevoice.modular.configuration_vibevoice import VibeVoiceConfig
    from vibevoice_rocm_amd import bnb
    from vibevoice_rocm_amd.modeling import VibeVoiceForConditionalGenerationInference as M
    from vibevoice_rocm_amd.modeling import load_prequantized_dir, save_checkpoint_dir
    cfg, sd = mid
    root = tmp_path_factory.mktemp("bnb4")
    save_checkpoint_dir(str(root / "bf16"), cfg, sd)
    names = write_bnb_dir(root / "repo" / "4bit", cfg, sd, which="all", blocksize=64, double=True, rest_dtype=torch.float16)
    try:
        from transformers import BitsAndBytesConfig
        qc = BitsAndBytesConfig(**REF_QC)
    except Exception:
        qc = dict(REF_QC)
    base_config = VibeVoiceConfig.from_pretrained(str(root / "bf16"))
    m = M.from_pretrained(str(root / "repo"), subfolder="4bit", config=base_config, quantization_config=qc, torch_dtype=torch.float16,
                          device_map="cuda", attn_implementation="sdpa", local_files_only=True)
    plain, recs = load_prequantized_dir(str(root / "repo" / "4bit"))
    assert set(recs) == set(names)
    return m, plain, recs, bnb.effective_state_dict(plain, recs)


def test_fork_call_vs_oracle(mid, fork_model):
    """Forced token schedule reproduced, audio within 2e-2 rel RMS of the oracle on the checkpoint's effective weights."""
    from oracle import vv_oracle as O
    cfg, _ = mid
    m, _, _, eff = fork_model
    assert m.weight_quant == "nf4" and m.dtype == torch.bfloat16
    sd_o = {k: (v.to(torch.bfloat16).float() if v.dim() >= 2 else v.float()) for k, v in eff.items()}     # the engine's bf16 matrices
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(11)
    ids = torch.randint(0, cfg.vocab - 8, (70,), generator=g)
    forced = [ST] + [D] * 5 + [E, EOS]
    noise = torch.randn(5, cfg.latent, generator=g)
    ref = O.generate(sd_o, cfg.as_dict(), ids.tolist(), torch.zeros(70, dtype=torch.bool), None, dict(speech_start=ST, speech_end=E,
                     speech_diffusion=D, eos=EOS), noise, cfg_scale=2.0, n_steps=10, forced_tokens=forced, bf16_t=True)
    out = _gen(m, cfg, ids, forced, noise)
    assert out.sequences[0, 70:].tolist() == forced
    got, want = out.speech_outputs[0][0].cpu().numpy(), torch.cat(ref.audio).numpy()
    assert got.shape == want.shape == (5 * cfg.hop,)
    err = rel_rms(got, want)
    assert err < 2e-2, f"pre-quantized nf4 generate() vs oracle on the effective weights: rel RMS {err:.3e}"


def test_fork_call_batch_of_3_on_lanes(mid, fork_model):
    """3 dialogues of the pre-quantized model run on the lock-step lanes and equal three single-dialogue calls bit for bit."""
    cfg, _ = mid
    m = fork_model[0]
    ST, E, D, EOS = _special(cfg)
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(0, cfg.vocab - 8, (3, 20), generator=g)
    forced = [[ST, D, D, D, E, EOS], [ST, D, E, EOS], [ST, D, D, E, ST, D, E, EOS]]
    noise = torch.randn(3, 4, cfg.latent, generator=g)
    m.set_ddpm_inference_steps(10)
    tok = _Tok(ST, E, D, EOS)
    out = m.generate(input_ids=ids, tokenizer=tok, cfg_scale=2.0, forced_tokens=forced, noise=noise)
    assert not m._rowbatch, "nf4 batch took the row-batched path"
    for b in range(3):
        one = m.generate(input_ids=ids[b:b + 1], tokenizer=tok, cfg_scale=2.0, forced_tokens=forced[b], noise=noise[b])
        assert torch.equal(one.speech_outputs[0].cpu(), out.speech_outputs[b].cpu()), f"dialogue {b}: lanes != single call"


def test_loaded_companions_preserve_the_file(mid, fork_model):
    """The VV_NF4 companions of the loaded model unpack to exactly the file's codes and decoded absmax (q | k | v fused), and the bf16 copies
    hold exactly the file's effective weights; matrices outside the companion set have bf16 copies only."""
    from vibevoice_rocm_amd import bnb
    from vibevoice_rocm_amd.weights import unpack_nf4
    cfg, _ = mid
    m, _, recs, eff = fork_model
    w = m.engine.w
    by_ptr = {t.data_ptr(): t for t in w._keep if isinstance(t, torch.Tensor)}

    def check(w8, ptr, keys):
        parts = [recs[k] for k in keys]
        n, k = sum(p.n for p in parts), parts[0].k
        codes, absmax = unpack_nf4(by_ptr[w8.q].cpu(), by_ptr[w8.scale].cpu(), n, k)
        assert torch.equal(codes, torch.cat([bnb.codes(p).view(p.n, p.k) for p in parts])), keys[0]
        assert torch.equal(absmax, torch.cat([bnb.block_absmax(p).view(p.n, p.k // 64) for p in parts])), keys[0]
        assert torch.equal(by_ptr[ptr].float().cpu(), torch.cat([eff[kk] for kk in keys])), keys[0]

    for l in range(cfg.layers):
        p, lay = f"model.language_model.layers.{l}.", w.llm.layer[l]
        check(lay.q_qkv, lay.wqkv, [p + f"self_attn.{c}_proj.weight" for c in "qkv"])
        for f, q, key in (("wo", "q_o", "self_attn.o_proj"), ("wgate", "q_gate", "mlp.gate_proj"), ("wup", "q_up", "mlp.up_proj"),
                          ("wdown", "q_down", "mlp.down_proj")):
            check(getattr(lay, q), getattr(lay, f), [p + key + ".weight"])
    for l in range(cfg.head_layers):
        p, lay = f"model.prediction_head.layers.{l}.", w.head.layer[l]
        for f, q, key in (("wgate", "q_gate", "ffn.gate_proj"), ("wup", "q_up", "ffn.up_proj"), ("wdown", "q_down", "ffn.down_proj")):
            check(getattr(lay, q), getattr(lay, f), [p + key + ".weight"])
    blk = w.dec.blocks[0][0]
    check(blk.q_w1, blk.w1, ["model.acoustic_tokenizer.decoder.stages.0.0.ffn.linear1.weight"])
    check(blk.q_w2, blk.w2, ["model.acoustic_tokenizer.decoder.stages.0.0.ffn.linear2.weight"])
    assert torch.equal(by_ptr[w.head.cond_proj].float().cpu(), eff["model.prediction_head.cond_proj.weight"])
    assert torch.equal(by_ptr[w.ac_conn.fc1].float().cpu(), eff["model.acoustic_connector.fc1.weight"])
