"""Records tests/golden/attention_routes.npz: the attention router's host queries (backward workspace bytes, uses-bf16 forward
and backward) over the grid tests/test_capi_cpu.py defines, answered by the library named on the command line.

  python tests/golden/make_attention_routes_golden.py PATH/TO/libgad_hip.so COMMIT

Run once against a library built from the commit the table stands for (the parent of the change it guards); the commit id is
stored with the table.  tests/test_capi_cpu.py::test_attention_route_table_matches_the_recorded_one checks the current build."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [os.path.join(ROOT, "group-attribution-for-diffusion-models_amd"), os.path.join(ROOT, "tests")]

from gad import _capi  # noqa: E402

if __name__ == "__main__":
    lib_path, commit = sys.argv[1], sys.argv[2]
    _capi.LIB_PATH = os.path.abspath(lib_path)
    import test_capi_cpu as T
    cols, _ = T.attention_route_table(_capi.load())
    out = os.path.join(HERE, "attention_routes.npz")
    np.savez_compressed(out, commit=np.array(commit), **cols)
    print(f"{out}: {len(cols['ws_bytes'])} cases, {os.path.getsize(out)} bytes, {(cols['ws_bytes'] > 0).sum()} with a workspace, "
          f"{cols['uses_bf16_bwd'].sum()} bf16")
