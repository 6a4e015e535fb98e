"""Record the launch policy of one build: tests/golden/launch_policy.rec (a numpy .npz archive; not named
.npz because test_oracle.py takes every *.npz of this directory for an oracle case).

    python tests/golden/make_policy_golden.py --pkg <checkout>/f110-mpc_amd --commit <its commit>

--pkg names the built package (lib/ and lib_test/ inside it) of the commit whose policy is the one to
keep: the commit BEFORE a change to the launch policy's code, never the tree under test. The file holds,
for every case of tests/policy_sweep.py, what that build's introspection calls answer (backend_info
ungrouped and grouped, lane_segments, lane_starts, lane_fixed_q, gap_screen), the sweep itself and the
commit. tests/test_launch_policy.py asserts that the current build answers the same. No device is needed.
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import policy_sweep as ps  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pkg", required=True, help="the f110-mpc_amd directory of the build to record")
    ap.add_argument("--commit", required=True, help="the commit that build was made from")
    args = ap.parse_args()
    sys.path.insert(0, os.path.abspath(args.pkg))
    from f110qp import capi

    assert os.path.abspath(capi.TEST_LIB_PATH).startswith(os.path.abspath(args.pkg)), capi.TEST_LIB_PATH
    assert capi.load(test=True).f110qp_test_build() == 1
    vs = ps.variants()
    out = np.zeros((len(vs), len(ps.HORIZONS), len(ps.BATCHES), ps.ANSWERS), np.int16)
    for i, v in enumerate(vs):
        for name in ps.KNOB_NAMES:
            os.environ.pop(name, None)
        if v["knob"]:
            os.environ[v["knob"][0]] = str(v["knob"][1])
        out[i] = ps.answers(capi, v)
    with open(os.path.join(HERE, "launch_policy.rec"), "wb") as f:
        np.savez_compressed(f, answers=out, variants=json.dumps(vs),
                            horizons=np.array(ps.HORIZONS), batches=np.array(ps.BATCHES), commit=args.commit)
    print(f"{out.shape} answers of {args.commit}: {len(np.unique(out.reshape(-1, ps.ANSWERS), axis=0))} distinct rows")


if __name__ == "__main__":
    main()
