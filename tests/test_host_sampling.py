"""Device-side do_sample, host half (no GPU): torch.multinomial(p, 1) on the CPU is argmax(p / q) over exponential draws q that do not depend on
p - the identity that lets the host draw q before it enqueues a step (batchloop.draw_q) - and batchloop.run under a recording fake driver draws
exactly those, where the host sampler draws, and leaves the generator where the host sampler leaves it."""
import itertools
import random

import torch

from test_host_cpu import _D, _E, _EOS, _ST, _FakeDriver, _run_loop


def test_argmax_p_over_q_is_multinomial_token_and_generator_state():
    """nv 4 / 5, logit scales 0.5 / 2 / 6, temperature 0.6 / 0.95 / 1.0 / 1.3, top_p 0.5 / 0.85 / 0.95 / 1.0, top_k 0 / 2 / 3 (288 settings x 12
    vectors = 3 456 cases, every sixth vector with a -inf logit): the token of modeling._make_sampler and torch.get_rng_state() after it equal
    those of q = draw_q(nv); ids[argmax(probs / q)] from the same seed."""
    from vibevoice_rocm_amd.batchloop import draw_q
    from vibevoice_rocm_amd.modeling import _make_sampler, _warped_probs
    g = torch.Generator().manual_seed(5)
    n = 0
    for nv, scale, temperature, top_p, top_k in itertools.product((4, 5), (0.5, 2.0, 6.0), (0.6, 0.95, 1.0, 1.3), (0.5, 0.85, 0.95, 1.0), (0, 2, 3)):
        cfg = dict(do_sample=True, temperature=temperature, top_p=top_p, top_k=top_k)
        sample, probs = _make_sampler(cfg), _warped_probs(cfg)
        ids = [100 + 3 * i for i in range(nv)]
        for rep in range(12):
            logits = (torch.randn(nv, generator=g) * scale).float()
            if rep % 6 == 5:
                logits[int(torch.randint(0, nv, (1,), generator=g))] = float("-inf")
            torch.manual_seed(1000 + n)
            want = sample(logits.clone(), ids)
            state = torch.get_rng_state()
            torch.manual_seed(1000 + n)
            q = draw_q(nv)
            got = ids[int(torch.argmax(probs(logits.clone()) / q))]
            assert got == want, (cfg, nv, logits, q)
            assert torch.equal(torch.get_rng_state(), state), (cfg, nv)
            n += 1
    assert n == 3456


class _SamplingDriver(_FakeDriver):
    """_FakeDriver whose unforced tokens come from a script (what the model would pick).  Host mode: calls sample_fn(logits, ids) once per live
    unforced dialogue in ascending order, as the lanes and the row batches do, and records the "logits" read.  Device mode: takes the draws q,
    must never see a sample_fn, and records what argmax(p / q) gives for the uniform p the host mode's sample_fn uses."""

    def __init__(self, script, **kw):
        super().__init__(**kw)
        self.script, self.draws, self.params, self.logit_reads = script, [], None, 0

    def set_sampler(self, temperature, top_k, top_p):
        self.params = (temperature, top_k, top_p)

    def _tokens(self, live, forced, sample_fn, q):
        toks = {}
        for b in live:
            if forced[b] is not None:
                assert q is None or b not in q
                toks[b] = forced[b]
                continue
            if q is None:
                self.logit_reads += 1
                self.draws.append((self.step, b, int(sample_fn(torch.zeros(4), [0, 1, 2, 3]))))
            else:
                assert sample_fn is None and q[b].shape == (4,) and q[b].dtype == torch.float32
                self.draws.append((self.step, b, int(torch.argmax(torch.full((4,), 0.25) / q[b]))))
            toks[b] = self.script[b][self.step]
        assert q is None or set(q) == {b for b in live if forced[b] is None}
        return toks

    def first_tokens(self, live, forced, sample_fn, q=None):
        self.step = 0
        return self._tokens(live, forced, sample_fn, q)

    def decode(self, live, forced, eligible, sample_fn, deliver, q=None):
        self.step += 1
        assert set(eligible) <= set(live) == set(forced)
        for b in eligible:
            self._rec("spec", b)
        deliver()
        self.deliveries += 1
        return self._tokens(live, forced, sample_fn, q), set(eligible)


def test_batch_loop_device_sampling_draws_where_the_host_sampler_draws(monkeypatch):
    """batchloop.run with BatchCall.sampler on random scripts of 2-4 dialogues, a third of the steps forced: one exponential_ per live unforced
    dialogue and step, in ascending order (counted on torch.Tensor.exponential_, and the outcomes argmax(p / q) equal the host sampler run's
    multinomial outcomes one by one); no logits are read and no sample_fn reaches the driver; frames are speculated (injected noise) and the
    mis-speculated ones rolled back, which the host-sampler run never does; and the generator ends where the host-sampler run's ends - with
    injected noise and with drawn noise (randn rows between the token draws), ODE and SDE.  (Batches speculate only with injected noise, so no
    draw of a speculated frame ever has to be taken back here; the single-dialogue loop, which does, is checked on the GPU.)"""
    calls = []
    real = torch.Tensor.exponential_

    def spy(self, *a, **k):
        calls.append(self.numel())
        return real(self, *a, **k)
    monkeypatch.setattr(torch.Tensor, "exponential_", spy)
    uniform = lambda logits, ids: ids[int(torch.multinomial(torch.full((4,), 0.25), 1))]      # noqa: E731
    rng = random.Random(3)
    rollbacks = spec = 0
    for it in range(150):
        B = rng.randint(2, 4)
        script = [[rng.choice([_D, _D, _D, _E, _ST]) for _ in range(rng.randint(1, 10))] + [_EOS] for _ in range(B)]
        forced = [[(t if rng.random() < 0.33 else None) for t in s] for s in script]
        sde = bool(it % 2)
        for inject in (True, False):
            kw = dict(noise=torch.zeros(B, 12, 4), sde_noise=torch.zeros(B, 12, 3, 4) if sde else None) if inject else {}
            host = _SamplingDriver(script, sde=sde)
            torch.manual_seed(it)
            n0 = len(calls)
            out_h, _, _ = _run_loop(forced, host, sample_fn=uniform, **kw)
            state_h = torch.get_rng_state()
            assert len(calls) == n0                      # multinomial draws inside the library: nothing goes through Tensor.exponential_
            dev = _SamplingDriver(script, sde=sde)
            torch.manual_seed(it)
            out_d, _, _ = _run_loop(forced, dev, sampler=(0.95, 0, 0.95), **kw)
            unforced = [(s, b) for s in range(max(map(len, script))) for b in range(B) if s < len(script[b]) and forced[b][s] is None]
            assert calls[n0:] == [4] * len(unforced)
            assert [d[:2] for d in dev.draws] == unforced == [d[:2] for d in host.draws]
            assert dev.draws == host.draws, (script, forced)
            assert torch.equal(torch.get_rng_state(), state_h), (script, forced, inject)
            assert out_d.sequences.tolist() == out_h.sequences.tolist()
            assert dev.params == (0.95, 0, 0.95) and dev.logit_reads == 0 and host.logit_reads == len(unforced)
            assert not [x for x in host.log if x[1] in ("spec", "rollback")]
            if inject:
                spec += len([x for x in dev.log if x[1] == "spec"])
                rollbacks += len([x for x in dev.log if x[1] == "rollback"])
            else:
                assert not [x for x in dev.log if x[1] in ("spec", "rollback")]
            assert [x for x in dev.log if x[1] == "speech" or x[1] == "spec"] or not any(_D in s for s in script)
    assert spec > 200 and rollbacks > 50, (spec, rollbacks)
