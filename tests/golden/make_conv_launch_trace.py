"""Records tests/golden/conv_launch_trace.json: what the convolution entries of gad/ops.py launch and ask the library, case by
case (tests/conv_launch_trace.py), traced on the CPU against the library named on the command line.

  python tests/golden/make_conv_launch_trace.py PATH/TO/libgad_hip.so COMMIT

Run once with the gad/ops.py of the commit the trace stands for (the parent of the change it guards); the commit id is stored
with the trace.  tests/test_conv_launch_cpu.py replays the cases against the current gad/ops.py."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), os.path.join(ROOT, "tests")]

from gad import _capi  # noqa: E402

if __name__ == "__main__":
    lib_path, commit = sys.argv[1], sys.argv[2]
    _capi.LIB_PATH = os.path.abspath(lib_path)
    import conv_launch_trace as T
    lib = _capi.load()
    cases = {name: T.run_case(lib, fn, hooked) for name, fn, hooked in T.CASES}
    out = os.path.join(HERE, "conv_launch_trace.json")
    with open(out, "w") as f:
        f.write('{"commit": %s, "cases": {\n' % json.dumps(commit))
        f.write(",\n".join(f"{json.dumps(name)}: {json.dumps(c, separators=(',', ':'))}" for name, c in cases.items()))
        f.write("\n}}\n")
    kids = sorted({l[-1][0] for c in cases.values() for l in c["launches"] if l[0] == "gad_gemm"})
    print(f"{out}: {len(cases)} cases, {sum(len(c['launches']) for c in cases.values())} launches, kernel ids {kids}, {os.path.getsize(out)} bytes")
