"""Records tests/golden/gemm_routes.npz: gad_gemm's five route queries (kernel id, plan tile / split / vec, workspace bytes,
Winograd bytes, uses-bf16) over the grid tests/test_capi_cpu.py defines, answered by the library named on the command line.

  python tests/golden/make_gemm_routes_golden.py PATH/TO/libgad_hip.so COMMIT

Run once against a library built from the commit the table stands for (the parent of the change it guards); the commit id is
stored with the table.  tests/test_capi_cpu.py::test_gemm_route_table_matches_the_recorded_one checks the current build."""
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
    cols, _ = T.gemm_route_table(_capi.load())
    out = os.path.join(HERE, "gemm_routes.npz")
    np.savez_compressed(out, commit=np.array(commit), **cols)
    print(f"{out}: {len(cols['kernel_id'])} cases, {os.path.getsize(out)} bytes, kernel ids {np.bincount(cols['kernel_id'] + 1)}")
