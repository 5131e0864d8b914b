"""batchloop.Session with packed_prefill under the recording fake driver of tests/test_host_session.py, on a machine without a GPU: requests
queued at once are admitted together - FIFO, lowest free slot first - and prefilled by ONE first_tokens call naming all their slots, and every
dialogue still receives exactly the driver calls batchloop.run makes for it alone."""
import random

import torch

from test_host_session import _D, _E, _EOS, _ST, _Fake, _alone, _request, _schedule, _session


class _FakeCalls(_Fake):
    """the fake, also recording each first_tokens call as the requests it names"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.first_calls = []

    def first_tokens(self, live, forced, sample_fn, q=None):
        assert list(live) == sorted(live) and set(live) == set(forced)
        self.first_calls.append([self.who[b] for b in live])
        return super().first_tokens(live, forced, sample_fn, q=q)


def test_queued_requests_share_one_first_tokens_call():
    """k requests queued before a step: one call with k slots (slots 0 .. k - 1 in submission order); the one-at-a-time session makes k calls.
    A request submitted mid-flight is admitted alone; five requests on four slots: four share a call, the fifth waits for a slot."""
    sch = [[_ST, _D, _D, _D, _E, _EOS], [_ST, _D, _D, _D, _D, _EOS], [_ST, _D, _D, _EOS]]
    for packed, want in ((True, [[0, 1, 2]]), (False, [[0], [1], [2]])):
        drv = _FakeCalls()
        sess = _session(drv, 4, True, packed_prefill=packed)
        hs = [sess.submit(_request(tag, 4, s, True, False, 3)) for tag, s in enumerate(sch)]
        assert sess.step() and [h.slot for h in hs] == [0, 1, 2]
        assert drv.first_calls == want and drv.order == [0, 1, 2]
        assert len(sess.admission_ms) == (1 if packed else 3) and [a[0] for a in sess.admissions] == [0, 1, 2]
        late = sess.submit(_request(3, 4, [_ST, _D, _EOS], True, False, 3))
        assert sess.step() and late.slot == 3 and drv.first_calls == want + [[3]]
        sess.run()
        assert all(h.done for h in hs + [late])
    drv = _FakeCalls()
    sess = _session(drv, 4, True, packed_prefill=True)
    hs = [sess.submit(_request(tag, 4, [_ST, _D, _D, _EOS], True, False, 3)) for tag in range(5)]
    sess.step()
    assert drv.first_calls == [[0, 1, 2, 3]] and hs[4].slot is None
    sess.run()
    assert drv.first_calls == [[0, 1, 2, 3], [4]] and drv.order == [0, 1, 2, 3, 4]


def test_a_first_token_that_ends_its_dialogue_frees_the_slot_in_the_same_step():
    """as the one-at-a-time admission: request 1 ends on its first token, so request 2 - which found no slot in the first wave - takes slot 1 in
    the same step, in a call of its own"""
    drv = _FakeCalls()
    sess = _session(drv, 2, True, packed_prefill=True)
    hs = [sess.submit(_request(tag, 4, s, True, False, 3)) for tag, s in enumerate([[_ST, _D, _D, _EOS], [_EOS], [_ST, _D, _EOS]])]
    assert sess.step()
    assert drv.first_calls == [[0, 1], [2]] and [h.slot for h in hs] == [0, 1, 1] and hs[1].done
    sess.run()
    assert drv.history == {0: [0], 1: [1, 2]}


def test_packed_session_equals_alone_and_the_unpacked_session():
    """Random scripts (arrivals in bursts, so waves of several requests are common): every dialogue's own record under packed admission equals
    batchloop.run's for it alone - which is what the session without the flag is held to - and its result is the same; admission stays FIFO."""
    rng = random.Random(31)
    waves = 0
    for it in range(80):
        slots, n_req = rng.randint(2, 8), rng.randint(6, 16)
        dn, sde, n_steps = bool(it % 2), bool((it // 2) % 2), 3
        drv = _FakeCalls(sde, n_steps)
        sess = _session(drv, slots, dn, packed_prefill=True)
        reqs, arrive = [], []
        for tag in range(n_req):
            sch = _schedule(rng)
            reqs.append(_request(tag, rng.randint(3, 9), sch, dn, sde, n_steps, max_length_times=rng.choice([2, 3, 50] if sch[-1] == _EOS else [2, 3])))
            arrive.append(rng.choice([0, 0, 3, 3, 7]))
        arrive.sort()
        handles, t = {}, 0
        while True:
            for tag in range(n_req):
                if arrive[tag] == t:
                    handles[tag] = sess.submit(reqs[tag])
            going = sess.step()
            t += 1
            if not going and t > arrive[-1]:
                break
            assert t < 2000
        sess.close()
        assert drv.order == list(range(n_req))
        assert sorted(tag for call in drv.first_calls for tag in call) == list(range(n_req))
        waves += sum(len(call) > 1 for call in drv.first_calls)
        for tag, req in enumerate(reqs):
            want_log, want = _alone(req, dn, sde, n_steps)
            got_log = [e[1:] for e in drv.log if e[0] == tag]
            assert got_log == want_log, (it, tag, req.forced_tokens, got_log, want_log)
            got = handles[tag].result()
            assert got.sequences.tolist() == want.sequences.tolist() and got.reach_max_step_sample.tolist() == want.reach_max_step_sample.tolist()
            if want.speech_outputs[0] is not None:
                assert torch.equal(got.speech_outputs[0], want.speech_outputs[0])
    assert waves >= 80, waves
