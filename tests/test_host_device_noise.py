"""Diffusion noise on the device, the parts a machine without a GPU can check: the generator's definition (tests/philox_ref.py, the reference
the GPU tests hold vv_noise_normal to) against the published known answers and the moments of a normal sample, the edge values of its
uniforms, and batchloop.run with BatchCall.noise_seeds under a recording driver - who is eligible for speculation, that the loop draws
nothing, and which frame index every frame carries."""
import ctypes as C
import random

import numpy as np
import torch

import philox_ref as P

_ST, _E, _D, _EOS, _PAD = 150, 151, 152, 153, 7


def test_philox_known_answers():
    """Philox4x32-10 known answers (Random123's kat_vectors: zero, all ones, the digits of pi)"""
    cases = [((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
             ((0xffffffff,) * 4, (0xffffffff,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
             ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), "d16cfe09 94fdcceb 5001e420 24126ea1")]
    for ctr, key, want in cases:
        assert " ".join("%08x" % int(v) for v in P.philox4x32_10(ctr, key)) == want, (ctr, key)
    # vectorised over the counter: the same words as one call per counter
    j = np.arange(5)
    x = P.philox4x32_10((j, 7, 1, 0), (3, 4))
    for i in range(5):
        assert [int(v[i]) for v in x] == [int(v) for v in P.philox4x32_10((i, 7, 1, 0), (3, 4))]


def test_reference_normals_have_normal_moments():
    """2^22 reference normals (one seed, frame 7, quads 0 .. 2^20 - 1): mean, variance and kurtosis inside five standard errors"""
    z = P.normal_quads(0x0123456789abcdef, 7, 0, np.arange(2 ** 20)).reshape(-1)
    N = z.size
    assert N == 2 ** 22 and np.isfinite(z).all()
    mean, var = z.mean(), z.var()
    kurt = ((z - mean) ** 4).mean() / var ** 2
    print(f"mean {mean * np.sqrt(N):.2f} se, var {(var - 1) / np.sqrt(2 / N):.2f} se, kurtosis {(kurt - 3) / np.sqrt(24 / N):.2f} se")
    assert abs(mean) < 5 / np.sqrt(N)
    assert abs(var - 1) < 5 * np.sqrt(2 / N)
    assert abs(kurt - 3) < 5 * np.sqrt(24 / N)


def test_uniform_edge_values():
    """x = 0 -> u = 2^-33 > 0 (log finite); x = 2^32 - 1 -> u == 1.0f exactly (r = 0, z finite)"""
    u = P.uniform(np.array([0, 0xffffffff, 1, 0x80000000]))
    assert u.dtype == np.float32
    assert u[0] == np.float32(2.0 ** -33) and u[0] > 0
    assert u[1] == np.float32(1.0)
    assert u[2] == np.float32(2.0 ** -32 + 2.0 ** -33) and u[3] == np.float32(0.5)
    assert (u > 0).all() and (u <= 1).all()
    for u0 in (u[0], u[1]):
        z = np.concatenate(P.box_muller(np.array([u0, u0]), np.array([u[0], u[1]])))
        assert np.isfinite(z).all()
    z0, z1 = P.box_muller(u[1], u[2])
    assert z0 == 0.0 and z1 == 0.0                                       # r(1) = 0
    assert abs(np.sqrt(-2 * np.log(float(u[0]))) - 6.7639) < 1e-3        # the largest radius there is


def test_abi_entry():
    from vibevoice_rocm_amd import _lib
    res, args = _lib.PROTOTYPES["vv_noise_normal"]
    assert res is C.c_int and args == [C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    assert hasattr(_lib.load(), "vv_noise_normal")


class _NoiseDriver:
    """Recording stand-in for the drivers behind batchloop.run with noise drawn on the device: returns the forced tokens, speculates every
    eligible dialogue and logs, per step, what it was handed.  log: (step, name, dialogue, frame index or None)."""
    sde, n_steps = True, 3

    def __init__(self):
        self.log, self.step, self.seeds, self.decodes = [], -1, None, []

    def begin(self, prompts, voices, max_steps, valid):
        self.began = True

    def set_noise_seeds(self, seeds):
        assert self.began and self.seeds is None
        self.seeds = list(seeds)

    def first_tokens(self, live, forced, sample_fn):
        self.step = 0
        return {b: forced[b] for b in live}

    def decode(self, live, forced, eligible, sample_fn, deliver):
        self.step += 1
        for b, row in eligible.items():
            assert isinstance(row, tuple) and len(row) == 2 and isinstance(row[0], int) and row[1] is None, row
            self.log.append((self.step, "spec", b, row[0]))
        self.decodes.append((self.step, list(live), set(eligible)))
        deliver()
        return {b: forced[b] for b in live}, set(eligible)

    def speech(self, rows):
        for b, row in rows.items():
            assert isinstance(row, tuple) and len(row) == 2 and isinstance(row[0], int) and row[1] is None, row
            self.log.append((self.step, "speech", b, row[0]))

    def chunk(self, b):
        self.log.append((self.step, "chunk", b, None))
        return torch.zeros(2)

    def synchronize(self):
        pass


for _name in ("replace_negative", "rollback", "reset_speech", "embed", "finished"):
    def _rec(self, b, *a, _name=_name):
        self.log.append((self.step, _name, b, None))
    setattr(_NoiseDriver, _name, _rec)


def _run(sch, driver, **kw):
    from vibevoice_rocm_amd import batchloop
    B = len(sch)
    L0 = [3 + b for b in range(B)]
    Lp = max(L0)
    ids = torch.full((B, Lp), _PAD, dtype=torch.long)
    am = torch.zeros(B, Lp, dtype=torch.long)
    for b in range(B):
        ids[b, Lp - L0[b]:] = torch.arange(10 + b, 10 + b + L0[b])
        am[b, Lp - L0[b]:] = 1
    call = batchloop.BatchCall(special=dict(speech_start=_ST, speech_end=_E, speech_diffusion=_D, eos=_EOS, bos=None), pad_id=_PAD, max_pos=4096,
                               latent=4, forced_tokens=[list(s) for s in sch], max_length_times=50, **kw)
    return batchloop.run(driver, ids, am, None, None, call), Lp


def _check(sch):
    B = len(sch)
    drv = _NoiseDriver()
    torch.manual_seed(3)
    state = torch.get_rng_state()
    out, Lp = _run(sch, drv, noise_seeds=[100 + b for b in range(B)])
    assert torch.equal(state, torch.get_rng_state()), sch                                   # the loop draws nothing
    assert drv.seeds == [100 + b for b in range(B)]
    for b in range(B):
        assert out.sequences[b, Lp:Lp + len(sch[b])].tolist() == sch[b]
    # every live dialogue whose previous token was speech_diffusion is eligible, and nobody else
    for step, live, elig in drv.decodes:
        assert live == [b for b in range(B) if len(sch[b]) > step], (sch, step, live)
        assert elig == {b for b in live if sch[b][step - 1] == _D}, (sch, step, elig)
    n_misspec = 0
    for b in range(B):
        mine = [(s, n, f) for s, n, b_, f in drv.log if b_ == b]
        kept, rolled = [], None
        for step in range(len(sch[b])):
            ev = [(n, f) for s, n, f in mine if s == step and n != "replace_negative"]
            spec = [f for n, f in ev if n == "spec"]
            rest = [(n, f) for n, f in ev if n != "spec"]
            assert len(spec) <= 1
            rb = [i for i, (n, _) in enumerate(rest) if n == "rollback"]
            if rb:
                assert spec and rb == [0], (sch, b, step, ev)                               # rollback first, and only after a speculation
                rolled = spec[0]
                n_misspec += 1
            elif spec:
                kept.append(spec[0])
                assert "speech" not in [n for n, _ in rest], (sch, b, step, ev)
            if spec and sch[b][step] != _D:
                assert rb, (sch, b, step, ev)
            sp = [f for n, f in rest if n == "speech"]
            assert len(sp) <= 1
            if sp:
                kept.append(sp[0])
            if (sp or (spec and not rb)) and rolled is not None:
                assert kept[-1] == rolled, (sch, b, step, kept, rolled)                      # the rolled-back index is the next real frame's
                rolled = None
            assert (sch[b][step] == _D) == bool(sp or (spec and not rb)), (sch, b, step, ev)
        assert kept == list(range(sch[b].count(_D))), (sch, b, kept)                         # 0, 1, 2, ...: no gap, no repeat
    return n_misspec


def test_batch_loop_with_noise_seeds_speculates_everyone_and_draws_nothing():
    """batchloop.run with noise_seeds: a turn switch in every dialogue, dialogue 1 ends early; then random schedules (restarts included)"""
    sch = [[_D, _D, _D, _E, _ST, _D, _D, _E, _EOS], [_D, _D, _E, _EOS], [_ST, _D, _D, _D, _E, _ST, _D, _EOS]]
    # rolled back: the frame speculated behind the last speech_diffusion of each run (2 + 1 + 2), and those of dialogues 0 and 1 at step 1,
    # where dialogue 2 diffuses for the first time next to them (_BatchCoupling: their conv states restart, the frame is redone)
    assert _check(sch) == 7
    rng = random.Random(23)
    hits = 0
    for _ in range(300):
        B = rng.randint(2, 4)
        hits += _check([[rng.choice([_D, _D, _D, _E, _ST]) for _ in range(rng.randint(1, 12))] + [_EOS] for _ in range(B)])
    assert hits > 300


def test_batch_loop_noise_seeds_refusals_and_default_path():
    """noise_seeds with injected noise, or of the wrong length, is refused; without noise_seeds the driver is never told about seeds"""
    import pytest
    sch = [[_D, _EOS], [_D, _EOS]]
    with pytest.raises(ValueError):
        _run(sch, _NoiseDriver(), noise_seeds=[1, 2], noise=torch.zeros(2, 4, 4))
    with pytest.raises(ValueError):
        _run(sch, _NoiseDriver(), noise_seeds=[1])

    class Plain(_NoiseDriver):
        sde = False

        def set_noise_seeds(self, seeds):
            raise AssertionError("not a device-noise call")

        def speech(self, rows):
            for b, (n_row, s_row) in rows.items():
                assert torch.is_tensor(n_row) and n_row.shape == (4,) and s_row is None

    _run(sch, Plain())
