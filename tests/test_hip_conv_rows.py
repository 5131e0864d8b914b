"""Row-batched conv tails (csrc/vv_conv_hot.hip; vv_decoder_front_rows, vv_decoder_forward_from, vv_encoder_forward_until,
vv_encoder_back_rows, vv_connector_pair_rows) against the per-dialogue composites they replace.

Component nets with the real widths and few blocks: the "mid" preset with 32 tokenizer filters, so the one-row stage is C = 2048 with two
blocks (depths 1, .., 1, 2) and both hand-over convs have their real shapes.  One root DeviceWeights plus forks: the batched path runs on one
set of forks, the per-dialogue composites on a twin set, both from zeroed state.

Figures of a GPU run (MI355X), relative RMS, dialogue 0, frames 0..2: per-dialogue path vs oracle 4.0e-3 .. 4.1e-3 (waveform) and
4.5e-3 .. 6.1e-3 (semantic feature); batched path vs oracle: the same figures, digit for digit; batched vs per-dialogue: waveform, semantic
feature and state blob are EQUAL, asserted with torch.equal at every B (the stem conv runs per dialogue; row_in_rows_kernel and rows_gemv_kernel
are one template each, the per-dialogue path runs their one-row instances, so row b has the one-row kernel's arithmetic by construction);
x rows 2.2e-7 at B = 2 and 3 and 1.1e-3 at B = 8: the connectors' B-row vv_linear calls take the m = B routes - another fp32
summation order at 2..3 rows; from 5 rows on the semantic connector's fc1 (K = 128, plain epilogue) is a shape of the skinny matrix-core kernel
(vv_skinny_covers, csrc/vv_convffn.hip), which rounds its activation rows to bf16 (2^-9 relative per element) - under the yardstick."""
import ctypes as C
import dataclasses

import pytest
import torch

from conftest import rel_rms

pytestmark = pytest.mark.gpu

ROW_BAR = 2e-2             # tests/test_hip_conv_hot.py, tests/test_hip_realshape.py: the bf16 bar of the one-row stage against the oracle
PRE_SCALE, PRE_BIAS = 0.5, 0.25
SENT = -77.0               # sentinel of rows that no store may reach
DEC, SEM = "model.acoustic_tokenizer.decoder.", "model.semantic_tokenizer.encoder."
E_ARG, E_UNSUPPORTED = -1, -3


def _cfg():
    from vibevoice_rocm_amd.config import VVConfig
    return dataclasses.replace(VVConfig.preset("mid"), ac_filters=32, ac_dec_filters=32, sem_filters=32)


def _latent(b, f, n):
    """dialogue b's latent of frame f: a function of (b, f) alone, so every B sees the same dialogue 0"""
    return torch.randn(n, generator=torch.Generator().manual_seed(1000 + 17 * b + f))


@pytest.fixture(scope="module")
def env():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from vibevoice_rocm_amd import _lib as L
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    from vibevoice_rocm_amd.weights import DeviceWeights
    lib = L.load()
    L.check(lib.vv_init(), "vv_init")
    cfg = _cfg()
    sd = synth_state_dict_torch(cfg, 77, device="cuda:0", dtype=torch.bfloat16)
    root = DeviceWeights(cfg, sd, "cuda:0")
    return dict(L=L, lib=lib, cfg=cfg, sd=sd, root=root)


@pytest.fixture(scope="module")
def oracle_d0(env):
    """dialogue 0's three frames on the CPU oracle (bf16-rounded weights, fp32 arithmetic), once for the module: [(wav, sem)]"""
    from oracle import vv_oracle as O
    cfg, sd = env["cfg"], env["sd"]
    Wd = {k: v.float().cpu() for k, v in sd.items() if k.startswith(DEC)}
    Ws = {k: v.float().cpu() for k, v in sd.items() if k.startswith(SEM)}
    torch.set_num_threads(16)
    st_d, st_s = O.ConvState(), O.ConvState()
    out = []
    for f in range(3):
        lat = _latent(0, f, cfg.ac_dim) * PRE_SCALE + PRE_BIAS
        wav = O.tokenizer_decoder(Wd, cfg.as_dict(), lat[:, None], st_d)[0]
        sem = O.semantic_encode(Ws, cfg.as_dict(), wav[None], st_s)[0]
        out.append((wav.clone(), sem.clone()))
    return out


class Rig:
    """B forks of one root with the buffers of both paths.  `batched(lat, mask)` runs one frame on the row-batched entry points,
    `single(lat, mask)` the per-dialogue composites for the active dialogues; the outputs land in wav / feat / x (sentinel-filled at reset)."""

    def __init__(self, env, root, B):
        L, lib, cfg = env["L"], env["lib"], env["cfg"]
        self.L, self.lib, self.cfg, self.B = L, lib, cfg, B
        self.w = [root.fork() for _ in range(B)]
        self.dec = (C.POINTER(L.ConvNet) * B)(*[C.pointer(w.dec) for w in self.w])
        self.sem = (C.POINTER(L.ConvNet) * B)(*[C.pointer(w.sem) for w in self.w])
        self.st = torch.cuda.Stream()
        f32 = dict(dtype=torch.float32, device="cuda:0")
        u8 = dict(dtype=torch.uint8, device="cuda:0")
        self.mid_n = 8 * 1024
        self.active = torch.ones(B, dtype=torch.int32, device="cuda:0")
        self.lat = torch.zeros(B, cfg.ac_dim, **f32)
        self.mid = torch.zeros(B, self.mid_n, **f32)
        self.mid2 = torch.zeros(B, self.mid_n, **f32)
        self.wav = torch.zeros(B, cfg.hop, **f32)
        self.feat = torch.zeros(B, cfg.sem_dim, **f32)
        self.x = torch.zeros(2 * B, cfg.hidden, **f32)
        fb = lib.vv_conv_rows_ws_bytes(C.byref(root.dec), B, 1)
        bb = lib.vv_conv_rows_ws_bytes(C.byref(root.sem), B, 0)
        assert fb > 0 and bb > 0
        self.front_ws = torch.empty(fb, **u8)
        self.back_ws = torch.empty(bb, **u8)
        self.dec_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(root.dec), 1, 1), **u8)
        self.sem_ws = torch.empty(lib.vv_convnet_ws_bytes(C.byref(root.sem), cfg.hop, 0), **u8)
        self.conn_ws = torch.empty(2 * B * cfg.hidden, **f32)
        self.reset()

    def reset(self):
        torch.cuda.synchronize()
        for w in self.w:
            w._state_arena.zero_()
        for t in (self.mid, self.mid2, self.wav, self.feat, self.x):
            t.fill_(SENT)
        torch.cuda.synchronize()

    def blobs(self):
        return [w.state_blob().clone() for w in self.w]

    def _set(self, lat, mask):
        self.lat.copy_(lat.cuda(), non_blocking=False)
        self.active.copy_(torch.tensor(mask, dtype=torch.int32).cuda())

    def front(self):
        L, lib, sp = self.L, self.lib, self.st.cuda_stream
        L.check(lib.vv_decoder_front_rows(self.dec, self.B, self.active.data_ptr(), self.lat.data_ptr(), self.lat.stride(0), PRE_SCALE, PRE_BIAS,
                                          self.mid.data_ptr(), self.mid_n, self.front_ws.data_ptr(), sp), "front")

    def middles(self, mask):
        L, lib, sp = self.L, self.lib, self.st.cuda_stream
        for b in range(self.B):
            if mask[b]:
                L.check(lib.vv_decoder_forward_from(C.byref(self.w[b].dec), self.mid[b].data_ptr(), self.wav[b].data_ptr(), self.dec_ws.data_ptr(), sp), "from")
                L.check(lib.vv_encoder_forward_until(C.byref(self.w[b].sem), self.wav[b].data_ptr(), self.cfg.hop, self.mid2[b].data_ptr(),
                                                     self.sem_ws.data_ptr(), sp), "until")

    def back(self):
        L, lib, sp, cfg = self.L, self.lib, self.st.cuda_stream, self.cfg
        r = self.w[0]
        L.check(lib.vv_encoder_back_rows(self.sem, self.B, self.active.data_ptr(), self.mid2.data_ptr(), self.mid_n, self.feat.data_ptr(), cfg.sem_dim,
                                         self.back_ws.data_ptr(), sp), "back")
        L.check(lib.vv_connector_pair_rows(C.byref(r.ac_conn), C.byref(r.sem_conn), self.lat.data_ptr(), self.lat.stride(0), self.feat.data_ptr(), cfg.sem_dim,
                                           self.active.data_ptr(), self.x.data_ptr(), cfg.hidden, 2, self.B, self.conn_ws.data_ptr(), sp), "connectors")

    def batched(self, lat, mask, front=None, back=None):
        self._set(lat, mask)
        with torch.cuda.stream(self.st):
            self.st.wait_stream(torch.cuda.default_stream())
            (front or self.front)()
            self.middles(mask)
            (back or self.back)()
        self.st.synchronize()

    def single(self, lat, mask):
        L, lib, sp, cfg = self.L, self.lib, self.st.cuda_stream, self.cfg
        self._set(lat, mask)
        with torch.cuda.stream(self.st):
            self.st.wait_stream(torch.cuda.default_stream())
            for b in range(self.B):
                if not mask[b]:
                    continue
                w = self.w[b]
                L.check(lib.vv_decoder_forward(C.byref(w.dec), self.lat[b].data_ptr(), 1, PRE_SCALE, PRE_BIAS, self.wav[b].data_ptr(), self.dec_ws.data_ptr(), sp), "dec")
                L.check(lib.vv_encoder_forward(C.byref(w.sem), self.wav[b].data_ptr(), cfg.hop, self.feat[b].data_ptr(), self.sem_ws.data_ptr(), sp), "sem")
                L.check(lib.vv_connector_pair(C.byref(w.ac_conn), C.byref(w.sem_conn), self.lat[b].data_ptr(), self.feat[b].data_ptr(), self.x[2 * b].data_ptr(),
                                              cfg.hidden, 2, self.conn_ws.data_ptr(), sp), "connectors")
        self.st.synchronize()

    def row_state(self, b):
        """(hist, hs) of every one-row block of dialogue b, decoder then encoder"""
        w, out = self.w[b], []
        base = w._state_arena.data_ptr()
        for net, stage in ((w.dec, 0), (w.sem, w.sem.n_stages - 1)):
            for j in range(net.n_blocks[stage]):
                blk = net.blocks[stage][j]
                for p, n in ((blk.hist, 6 * 2048), (blk.hs, 2048)):
                    o = (p - base) // 4
                    out.append(w._state_arena[o: o + n].clone())
        return out


def _lats(cfg, B, f, salt=0):
    return torch.stack([_latent(b + salt * (b != 2), f, cfg.ac_dim) for b in range(B)])


def _subset(B):
    m = [1] * B
    for b in range(1, B, 2):        # dialogue 0 stays, dialogue 1 leaves: at least one of each
        m[b] = 0
    return m


@pytest.mark.parametrize("B", [2, 3, 6, 7, 8])       # 6, 7: the 2048 x 16384 hand-over in passes of 3 and of 2 rows, 7 with a partial last pass
def test_rows_vs_per_dialogue_composites(env, oracle_d0, B):
    cfg = env["cfg"]
    rows, twin = Rig(env, env["root"], B), Rig(env, env["root"], B)
    masks = [[1] * B, _subset(B), [1] * B]
    for f, mask in enumerate(masks):
        lat = _lats(cfg, B, f)
        for t in (rows.mid, rows.mid2, rows.wav, rows.feat, rows.x):     # every output row holds the sentinel: any store to an inactive dialogue shows
            t.fill_(SENT)
        before = rows.blobs()
        rows.batched(lat, mask)
        twin.single(lat, mask)
        after = rows.blobs()
        tb = twin.blobs()
        wav_ref, sem_ref = oracle_d0[f]
        # the yardstick: the per-dialogue path's own error against the oracle (dialogue 0 is active in every frame), in this run
        yw = rel_rms(twin.wav[0].cpu().numpy(), wav_ref.numpy(), what=f"per-dialogue wav vs oracle B={B} f={f}")
        ys = rel_rms(twin.feat[0].cpu().numpy(), sem_ref.numpy(), what=f"per-dialogue sem vs oracle B={B} f={f}")
        bw = rel_rms(rows.wav[0].cpu().numpy(), wav_ref.numpy(), what=f"batched wav vs oracle B={B} f={f}")
        bs = rel_rms(rows.feat[0].cpu().numpy(), sem_ref.numpy(), what=f"batched sem vs oracle B={B} f={f}")
        print(f"B={B} frame {f}: per-dialogue vs oracle wav {yw:.3e} sem {ys:.3e}; batched vs oracle wav {bw:.3e} sem {bs:.3e}")
        assert yw < ROW_BAR and ys < ROW_BAR, "the yardstick itself"
        assert bw < ROW_BAR and bs < ROW_BAR, (bw, bs)
        for b in range(B):
            if not mask[b]:
                assert torch.equal(after[b], before[b]), f"inactive dialogue {b}: state written"
                for t in (rows.mid[b], rows.mid2[b], rows.wav[b], rows.feat[b], rows.x[2 * b: 2 * b + 2]):
                    assert torch.equal(t, torch.full_like(t, SENT)), f"inactive dialogue {b}: output row written"
                continue
            # one kernel template for one row and for B rows: waveform, semantic feature and state are the per-dialogue path's, bit for bit
            assert torch.equal(rows.wav[b], twin.wav[b]), f"B={B} f={f} b={b}: waveform differs from the per-dialogue path"
            assert torch.equal(rows.feat[b], twin.feat[b]), f"B={B} f={f} b={b}: semantic feature differs from the per-dialogue path"
            assert torch.equal(after[b], tb[b]), f"B={B} f={f} b={b}: state blob differs from the per-dialogue path"
            # the connector rows: another summation order at m = B (module docstring), under the yardstick
            dx = rel_rms(rows.x[2 * b: 2 * b + 2].cpu().numpy(), twin.x[2 * b: 2 * b + 2].cpu().numpy(), what=f"batched vs per-dialogue x B={B} f={f} b={b}")
            if b == 0:
                print(f"  dialogue 0 batched vs per-dialogue: wav, sem and state equal, x {dx:.3e}")
            assert dx < ys, (b, dx, ys)
            assert torch.equal(rows.x[2 * b], rows.x[2 * b + 1])


def test_bit_exact_core_with_the_ffn_switched_off(env):
    """ffn_gamma = 0 in the one-row blocks takes the FFN out of the chain: what is left - stem / hand-over conv, the mixers, both RMSNorms, the
    history shift and hs - must equal the per-dialogue path bit for bit"""
    from vibevoice_rocm_amd.weights import DeviceWeights
    cfg = env["cfg"]
    sd = dict(env["sd"])
    for j in range(2):
        for k in (f"{DEC}stages.0.{j}.ffn_gamma", f"{SEM}stages.6.{j}.ffn_gamma"):
            assert k in sd
            sd[k] = torch.zeros_like(sd[k])
    root = DeviceWeights(cfg, sd, "cuda:0")
    B = 3
    rows, twin = Rig(env, root, B), Rig(env, root, B)
    for f in range(2):
        lat = _lats(cfg, B, f)
        rows.batched(lat, [1] * B)
        twin.single(lat, [1] * B)
    for b in range(B):
        got, want = rows.row_state(b), twin.row_state(b)
        assert len(got) == 8                 # (hist, hs) x 2 blocks x 2 nets
        for i, (g, w) in enumerate(zip(got, want)):
            assert float(w.abs().max()) > 0 and torch.equal(g, w), (b, i)


def test_independence_and_determinism(env):
    cfg, B = env["cfg"], 5
    rig = Rig(env, env["root"], B)

    def run(salt, masks):
        rig.reset()
        for f, mask in enumerate(masks):
            rig.batched(_lats(cfg, B, f, salt), mask)
        return [t.clone() for t in (rig.wav[2], rig.feat[2], rig.x[4:6], rig.w[2].state_blob())]

    a = run(0, [[1] * B, [1, 0, 1, 1, 0]])
    b = run(1, [[1, 1, 1, 0, 1], [0, 1, 1, 0, 0]])          # the other dialogues' inputs and masks differ
    c = run(0, [[1] * B, [1, 0, 1, 1, 0]])                  # a plain repeat
    for i in range(4):
        assert torch.equal(a[i], b[i]), f"dialogue 2 depends on its neighbours ({i})"
        assert torch.equal(a[i], c[i]), f"not deterministic ({i})"


def test_graph_replay_equals_eager(env):
    cfg, B = env["cfg"], 4
    L, lib = env["L"], env["lib"]
    eager, graphed = Rig(env, env["root"], B), Rig(env, env["root"], B)
    graphs = []
    for fn in (graphed.front, graphed.back):
        graphed.st.synchronize()
        L.check(lib.vv_graph_begin(graphed.st.cuda_stream), "begin")
        with torch.cuda.stream(graphed.st):
            fn()
        ge = C.c_void_p()
        L.check(lib.vv_graph_end(graphed.st.cuda_stream, C.byref(ge)), "end")
        graphs.append(ge)
    replay = [lambda g=g: L.check(lib.vv_graph_launch(g, graphed.st.cuda_stream), "launch") for g in graphs]
    try:
        for f, mask in enumerate([[1, 1, 1, 1], [0, 1, 0, 1], [1, 0, 1, 1]]):
            lat = _lats(cfg, B, f)
            eager.batched(lat, mask)
            graphed.batched(lat, mask, front=replay[0], back=replay[1])
            for name in ("mid", "wav", "feat", "x"):
                assert torch.equal(getattr(eager, name), getattr(graphed, name)), (f, name)
            for b, (p, q) in enumerate(zip(eager.blobs(), graphed.blobs())):
                assert torch.equal(p, q), (f, b)
        assert float(eager.x[0].abs().max()) > 0 and float(eager.x[2, 0]) != SENT
    finally:
        torch.cuda.synchronize()
        for g in graphs:
            lib.vv_graph_destroy(g)


def test_refusals_come_before_any_launch(env):
    from vibevoice_rocm_amd.config import VVConfig
    from vibevoice_rocm_amd.synth import synth_state_dict_torch
    from vibevoice_rocm_amd.weights import DeviceWeights
    L, lib, cfg, root = env["L"], env["lib"], env["cfg"], env["root"]
    rig = Rig(env, root, 2)

    def nets(ws, attr, n):
        return (C.POINTER(L.ConvNet) * n)(*[C.pointer(getattr(ws[i % len(ws)], attr)) for i in range(n)])

    def front(arr, B, ws=None):
        return lib.vv_decoder_front_rows(arr, B, rig.active.data_ptr(), rig.lat.data_ptr(), rig.lat.stride(0), 1.0, 0.0, rig.mid.data_ptr(), rig.mid_n,
                                         (ws or rig.front_ws).data_ptr(), None)

    def back(arr, B):
        return lib.vv_encoder_back_rows(arr, B, rig.active.data_ptr(), rig.mid2.data_ptr(), rig.mid_n, rig.feat.data_ptr(), cfg.sem_dim,
                                        rig.back_ws.data_ptr(), None)

    nine = [root.fork() for _ in range(9)]
    for B in (1, 9):
        assert front(nets(nine, "dec", 9), B) == E_UNSUPPORTED and back(nets(nine, "sem", 9), B) == E_UNSUPPORTED
        assert lib.vv_conv_rows_ws_bytes(C.byref(root.dec), B, 1) == 0
        assert lib.vv_connector_pair_rows(C.byref(root.ac_conn), C.byref(root.sem_conn), rig.lat.data_ptr(), cfg.ac_dim, rig.feat.data_ptr(), cfg.sem_dim,
                                          rig.active.data_ptr(), rig.x.data_ptr(), cfg.hidden, 2, B, rig.conn_ws.data_ptr(), None) == E_UNSUPPORTED
    # a net of another width: the plain "mid" preset's one-row stage is C = 512
    narrow_cfg = VVConfig.preset("mid")
    narrow = DeviceWeights(narrow_cfg, synth_state_dict_torch(narrow_cfg, 5, device="cuda:0", dtype=torch.bfloat16), "cuda:0")
    nf = [narrow.fork() for _ in range(2)]
    assert front(nets(nf, "dec", 2), 2) == E_UNSUPPORTED and back(nets(nf, "sem", 2), 2) == E_UNSUPPORTED
    assert lib.vv_conv_rows_ws_bytes(C.byref(narrow.dec), 2, 1) == 0
    # fp8 companions on the one-row blocks
    q = DeviceWeights(cfg, env["sd"], "cuda:0", quant="fp8")
    qf = [q.fork() for _ in range(2)]
    assert front(nets(qf, "dec", 2), 2) == E_UNSUPPORTED and back(nets(qf, "sem", 2), 2) == E_UNSUPPORTED
    # nets with different weights: two roots built from the same state dict hold their own device copies
    other = DeviceWeights(cfg, env["sd"], "cuda:0")
    mixed = [rig.w[0], other.fork()]
    assert front(nets(mixed, "dec", 2), 2) == E_ARG and back(nets(mixed, "sem", 2), 2) == E_ARG
    # one fork twice: two dialogues on one state
    assert front(nets([rig.w[0]], "dec", 2), 2) == E_ARG
    # null pointers
    assert lib.vv_decoder_front_rows(rig.dec, 2, None, rig.lat.data_ptr(), cfg.ac_dim, 1.0, 0.0, rig.mid.data_ptr(), rig.mid_n, rig.front_ws.data_ptr(), None) == E_ARG
    assert lib.vv_decoder_forward_from(C.byref(rig.w[0].dec), None, rig.wav.data_ptr(), rig.dec_ws.data_ptr(), None) == E_ARG
    assert lib.vv_encoder_forward_until(C.byref(rig.w[0].sem), rig.wav.data_ptr(), cfg.hop, None, rig.sem_ws.data_ptr(), None) == E_ARG
    assert b"fork" in lib.vv_last_error() or b"null" in lib.vv_last_error()
    torch.cuda.synchronize()
    for t in (rig.mid, rig.mid2, rig.wav, rig.feat, rig.x):
        assert bool((t == SENT).all()), "a refused call wrote an output"
    for w in rig.w:
        assert float(w.state_blob().abs().max()) == 0.0, "a refused call wrote state"
