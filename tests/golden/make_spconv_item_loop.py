"""Writes tests/golden/spconv_item_loop.npz: the outputs of the hand-made rulebooks of tests/test_gpu_spconv_item_loop.py, as the library
built from the commit given on the command line computes them (needs the GPU).  Run it with the PARENT of a change that must keep the
bits, from the repository root:

    python tests/golden/make_spconv_item_loop.py <commit id> [output file]

Per case: "in:<key>" the digest of the generated inputs, "sha:<key>" the digest of the output, "out:<key>" the output itself for the
cases of up to 129 rows (the 300-row cases are recorded by digest alone, to keep the file small)."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))                   # tests/
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))  # the repository root


def main():
    import test_gpu_spconv_item_loop as T
    from futuredet_amd import build, hip_ops, lib

    commit = sys.argv[1]
    out = sys.argv[2] if len(sys.argv) > 2 else T.GOLDEN
    build.build()
    lib.load()
    z = {"commit": np.array(commit)}
    for variant in T.VARIANTS:
        for cin, cout in T.FAMILIES:
            for n_out in T.N_OUT:
                case = T.make_case(hip_ops, variant, cin, cout, n_out)
                y = T.golden_call(hip_ops, case)
                # every other route of the parent carries the same bits: what the test will ask of the new build
                for name, yr in T.routes(hip_ops, case):
                    assert T.digest(yr) == T.digest(y), name
                z["in:" + case["key"]] = np.array(T.input_digest(case))
                z["sha:" + case["key"]] = np.array(T.digest(y))
                if n_out <= T.GOLDEN_FULL_ROWS and variant == "edges":
                    z["out:" + case["key"]] = y.cpu().numpy()
    os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
    np.savez(out, **z)
    print("wrote %s: %d cases, %d bytes" % (out, (len(z) - 1) // 2, os.path.getsize(out)))


if __name__ == "__main__":
    main()
