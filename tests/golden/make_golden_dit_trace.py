"""Writes tests/golden/dit_call_trace.json: for every case of tests/dit_trace.py the C entry points a LightningDiT forward / backward calls,
in order, with their scalars and the null / non-null pattern of their pointers -- one call per line.  Needs an MI355X.

    python tests/golden/make_golden_dit_trace.py [--tensors DIR]

The file was generated at the parent of the commit that gave models/lightningdit.py one block backward and one attention front end, so it
records the launches of the code BEFORE that change and not those of the code under test; tests/test_gpu_dit_trace.py holds every later
version to it.  A change that alters launches ON PURPOSE regenerates it: run this script on the changed tree with none of
dit_trace.SWITCHES set, read the diff of the JSON file -- every line in it must be a launch the change means to add, drop or alter -- and
commit the file together with the change, saying so in the commit message.

Before writing, each case is checked to have reached the branch it is named for (dit_trace.check_branch).  --tensors DIR also saves each
case's output, dx and every parameter gradient to DIR/<case>.npz, for a bitwise comparison of two versions of the module run on one
machine; nothing of that is committed."""
import argparse
import json
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)

import dit_trace as T      # noqa: E402


def dumps(traces):
    parts = []
    for cid, log in traces.items():
        parts.append(json.dumps(cid) + ": [\n" + ",\n".join(json.dumps(e) for e in log) + "\n]")
    return "{\n" + ",\n".join(parts) + "\n}\n"


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--tensors", metavar="DIR")
    ap.add_argument("--out", default=os.path.join(HERE, "dit_call_trace.json"))
    args = ap.parse_args(argv)
    assert T.switch_set() is None, f"{T.switch_set()} is set: the golden trace is that of the default environment"
    traces = {}
    for case in T.CASES:
        log, got = T.run_case(case)
        T.check_branch(case, log)
        traces[case["id"]] = log
        print(f"{case['id']}: {len(log)} calls, {len(got)} tensors")
        if args.tensors:
            os.makedirs(args.tensors, exist_ok=True)
            np.savez(os.path.join(args.tensors, case["id"] + ".npz"), **{k: v.detach().float().cpu().numpy() for k, v in got.items()})
    text = dumps(traces)
    assert json.loads(text) == traces
    with open(args.out, "w") as f:
        f.write(text)
    print(f"wrote {args.out}: {sum(len(v) for v in traces.values())} calls in {len(traces)} cases")


if __name__ == "__main__":
    main()
