#!/usr/bin/env python
"""What vv_linear_route answers over a grid of calls: (rc, route name) per case, recorded to and compared with tests/golden/linear_route_sweep.json.

Host decisions only: the arguments are built from stand-in addresses, vv_linear is never called and nothing is launched.  The grid is the
product of the CORE axes (weight dtype, rows, shape, SwiGLU pair, one flag) with the other axes varied one at a time around an aligned call
with both scale arrays: a missing wscale / w2scale, each operand 4 and 8 bytes off, a row pitch of k + 2 and the broadcast pitch 0.

    python tools/route_sweep.py --record tests/golden/linear_route_sweep.json            # the "off" half: no rows scratch, no GPU needed
    python tools/route_sweep.py --record tests/golden/linear_route_sweep.json --scratch  # the "on" half (m >= 3), needs the GPU: the scratch is device memory
    python tools/route_sweep.py --check tests/golden/linear_route_sweep.json [--scratch]

The record keeps both halves whole (121 k decisions) in 19 KB: the route names as a list, the per-case results and stages packed (load / save).
Each refused case also carries the stage that refused it, found by asking again with the fault repaired (never from the message): "l" = taken
once every operand is aligned and the pitch is k, "k" = a k of whole 128s that is taken at k = 1024 (the row was beyond the format's kernels),
"a" = everything else (shape, flags, scales, dtype)."""
import argparse
import base64
import ctypes as C
import itertools
import json
import os
import struct
import sys
import zlib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

WDT = (0, 1, 2, 3, 4, 5, 6, 7)               # VV_F32 .. VV_MXFP6, and 7: no such dtype
ROWS = (1, 2, 3, 4, 8, 9, 16)
SHAPES = ((32, 1024), (24, 1024), (32, 1056), (32, 1040), (1536, 8960), (32, 20992), (32, 26624))     # (n, k)
FLAGS = (0, 8, 1, 2, 32)                     # none, VV_LIN_W_FRAG, VV_LIN_X_BF16, VV_LIN_OUT_BF16, VV_LIN_W_MXGEMM
_ADDR = {name: 0x10000000 * (i + 1) for i, name in enumerate(("x", "w", "w2", "norm_w", "shift", "scale", "out", "wscale", "w2scale"))}
# the one-at-a-time variants: (wscale present, w2scale present, {operand: byte offset}, prologue, pitch) - prologue 0 none, 1 RMSNorm, 2 RMSNorm + adaLN rows;
# pitch "k", "k+2" or 0
_BASE = (1, 1, {}, 0, "k")
VARIANTS = ([_BASE, (0, 1, {}, 0, "k"), (1, 0, {}, 0, "k"), (0, 0, {}, 0, "k")]
            + [(1, 1, {p: off}, 0, "k") for p in ("w", "w2", "wscale", "x") for off in (4, 8)]
            + [(1, 1, {"norm_w": off}, 1, "k") for off in (0, 4, 8)]
            + [(1, 1, {"shift": off, "scale": off}, 2, "k") for off in (0, 4, 8)]
            + [(1, 1, {}, 0, "k+2"), (1, 1, {}, 0, 0)])


def cases(min_rows=1):
    """Every case as (wdt, m, (n, k), dual, flag, variant), in the order the record keeps."""
    for wdt, m, nk, dual, flag in itertools.product(WDT, ROWS, SHAPES, (0, 1), FLAGS):
        if m < min_rows:
            continue
        for v in VARIANTS:
            if not dual and (not v[1] or "w2" in v[2]):
                continue                      # w2 and its scales exist on SwiGLU pairs only
            yield wdt, m, nk, dual, flag, v


def lin_args(L, case, repair=0):
    """The call of a case; repair 1: every operand aligned and the pitch k, 2: also k = 1024"""
    wdt, m, (n, k), dual, flag, (ws, w2s, offs, pro, pitch) = case
    if repair:
        offs, pitch = {}, "k"
    if repair == 2:
        k = 1024
    at = lambda name: _ADDR[name] + offs.get(name, 0)
    a = L.LinArgs()
    a.x, a.m, a.n, a.k, a.wdt, a.w, a.out, a.ldo, a.flags, a.eps = at("x"), m, n, k, wdt, at("w"), _ADDR["out"], n, flag, 1e-6
    a.ldx = {"k": k, "k+2": k + 2, 0: 0}[pitch]
    if ws:
        a.wscale = at("wscale")
    if dual:
        a.w2, a.act = at("w2"), L.ACT_SWIGLU
        if w2s:
            a.w2scale = at("w2scale")
    if pro:
        a.pro, a.norm_w = L.PRO_RMSNORM, at("norm_w")
    if pro == 2:
        a.mod_shift, a.mod_scale, a.ld_mod = at("shift"), at("scale"), 3 * k
    return a


def sweep(L, lib, min_rows=1, classify=True):
    """-> (names, results, stages, messages): results[i] >= 0 indexes names (rc 0), < 0 is the refusal's rc; stages[i] in ".alk" ("a" for every
    refusal without classify, which spares the repeated queries); messages[i]: was vv_last_error() non-empty after a refusal (True for a taken call)"""
    buf = C.create_string_buffer(192)

    def ask(case, repair=0):
        a = lin_args(L, case, repair)
        return lib.vv_linear_route(C.byref(a), buf, 192)

    names, index, results, stages, said = [], {}, [], [], []
    for case in cases(min_rows):
        rc = ask(case)
        if rc == 0:
            name = buf.value.decode()
            if name not in index:
                index[name] = len(names)
                names.append(name)
            results.append(index[name])
            stages.append(".")
            said.append(True)
            continue
        said.append(bool(lib.vv_last_error()))
        results.append(rc)
        stages.append("a" if not classify else "l" if ask(case, 1) == 0 else "k" if case[2][1] % 128 == 0 and ask(case, 2) == 0 else "a")
    return names, results, "".join(stages), said


def _lib(scratch):
    from vibevoice_rocm_amd import _lib as L
    lib = L.load()
    if scratch:
        L.check(lib.vv_init(), "vv_init")
    return L, lib


def run(scratch, classify=True):
    """The half of the record this process can give: scratch off, every case; on, the cases of 3 rows and more (the scratch is switched off again)"""
    L, lib = _lib(scratch)
    if not scratch:
        return sweep(L, lib, classify=classify)
    L.check(lib.vv_tune(b"gemv_rows_scratch", 1), "vv_tune")
    try:
        return sweep(L, lib, min_rows=3, classify=classify)
    finally:
        lib.vv_tune(b"gemv_rows_scratch", 0)


def _pack(data: bytes) -> str:
    return base64.b64encode(zlib.compress(data, 9)).decode()


def _unpack(text: str) -> bytes:
    return zlib.decompress(base64.b64decode(text))


def load(path):
    """The record as {half: {"min_rows", "names", "results" (list of int), "stages" (str)}}.  In the file a half's results are little-endian
    int16, one per case in cases() order, and its stages one character per case, both zlib-compressed and base64-encoded: the runs are long."""
    rec = json.load(open(path)) if os.path.exists(path) else {}
    return {half: {"min_rows": h["min_rows"], "names": h["names"], "stages": _unpack(h["stages"]).decode(),
                   "results": struct.unpack(f"<{h['cases']}h", _unpack(h["results"]))} for half, h in rec.items()}


def save(path, rec):
    out = {half: {"min_rows": h["min_rows"], "cases": len(h["results"]), "names": h["names"], "stages": _pack(h["stages"].encode()),
                  "results": _pack(struct.pack(f"<{len(h['results'])}h", *h["results"]))} for half, h in rec.items()}
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")


def compare(rec, got):
    """The differences between a recorded half and a fresh one, as readable lines (at most 20)"""
    names, results, stages, said = got
    diffs = []
    if len(results) != len(rec["results"]):
        return [f"{len(results)} cases now, {len(rec['results'])} recorded: the grid changed, record it again at the parent commit"]
    show = lambda r, nm: nm[r] if r >= 0 else f"rc {r}"
    for i, (case, want, have) in enumerate(zip(cases(rec["min_rows"]), rec["results"], results)):
        if show(want, rec["names"]) != show(have, names):
            diffs.append(f"{case}: recorded {show(want, rec['names'])}, now {show(have, names)}")
        elif not said[i]:
            diffs.append(f"{case}: refused (rc {have}) without a message")
        if len(diffs) >= 20:
            break
    return diffs


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--record", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--scratch", action="store_true", help="the half with vv_tune('gemv_rows_scratch', 1): m >= 3, needs the GPU")
    o = ap.parse_args()
    half = "scratch_on" if o.scratch else "scratch_off"
    got = run(o.scratch)
    names, results, stages, said = got
    path = o.record or o.check
    rec = load(path) if path else {}
    if o.record:
        rec[half] = {"min_rows": 3 if o.scratch else 1, "names": names, "results": results, "stages": stages}
        save(o.record, rec)
    taken = sum(r >= 0 for r in results)
    print(f"{half}: {len(results)} cases, {taken} taken on {len(names)} routes, refused: " +
          ", ".join(f"{s}={stages.count(s)}" for s in "alk") + f", silent refusals: {said.count(False)}")
    if o.check:
        diffs = compare(rec[half], got)
        print("\n".join(diffs) if diffs else "no difference")
        return 1 if diffs else 0
    return 0


if __name__ == "__main__":
    sys.exit(main())
