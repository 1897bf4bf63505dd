#!/usr/bin/env python
"""Makes tests/golden/frontend_refusals.json: what the front ends' entry points answer to the deliberately bad calls of
tests/refusal_cases.py - per case the return code and, for an entry point with a context, the text cvo_last_error holds -
and what the matcher's, the filter's and the stereo front end's stats read after a successful pair call and after the
refused calls behind it.

    python scripts/make_refusal_golden.py [--out FILE] [--lib libcvo_hip.so]

Run it on the commit whose behaviour is to be kept, BEFORE changing the entry points: the record is the reference of
tests/test_frontend_refusals.py and tests/test_gpu_frontend_refusals.py, never the code under test.  The cases with a context
need a GPU (nothing is launched but by the one successful call of the stats check); without one only the twins' half is
recorded and the other half of an existing file stays as it is."""
import argparse
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    sys.path.insert(0, p)
import refusal_cases as rc  # noqa: E402
from unified_cvo_amd import _capi  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "frontend_refusals.json"))
    ap.add_argument("--lib", default=None)
    a = ap.parse_args()
    L = _capi.lib(a.lib)
    record = json.load(open(a.out)) if os.path.exists(a.out) else dict(cases={}, stats={})
    ctx = C.c_void_p()
    have_gpu = L.cvo_ctx_create(0, C.byref(ctx)) == 0
    done = 0
    for case in rc.cases():
        if case.ctx and not have_gpu:
            continue
        print(case.name, flush=True)  # (a case that is not refused may crash on its pointers: the last line names it)
        got = rc.run(L, ctx, case)
        assert got["rc"] != 0, f"{case.name} is not refused"
        record["cases"][case.name] = got
        done += 1
    if have_gpu:
        record["stats"] = rc.survival(L, ctx)
        assert record["stats"]["after_success"] == record["stats"]["after_refusals"], "a refused call changed the stats"
        L.cvo_ctx_destroy(ctx)
    stale = set(record["cases"]) - {c.name for c in rc.cases()}
    for name in stale:
        del record["cases"][name]
    with open(a.out, "w") as f:
        json.dump(record, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{a.out}: {done} cases recorded ({'with' if have_gpu else 'WITHOUT'} the context entry points), {os.path.getsize(a.out)} bytes")


if __name__ == "__main__":
    main()
