"""Child process of tests/test_gpu_pca_kernels.py: the PCA products in ANOTHER kernel form.  csrc/gram.hip reads VCY_GRAM_DMA and
VCY_GEMM_NT_SHAPE once per process, so the parent sets one of them in this process's environment and checks what comes back.

    python tests/pca_products_worker.py OUT.npz gram|gemm_nt

Runs pca_cases.worker_gram_jobs() or worker_gemm_jobs() through velocyto_amd.ops and writes every result under pca_cases.key(...).  With
VCY_GEMM_NT_SHAPE = 2 or 3 it also calls vcy_gemm_nt with row pitches that hold whole 128-byte but not whole 256-byte slab rows and
records the return code and message (the documented refusal), and the untouched output."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)


def main(out_path, what):
    import torch
    import velocyto_amd  # noqa: F401
    from velocyto_amd import ops
    import pca_cases as pc
    dev = ops.require_gpu()
    out = {}
    if what == "gram":
        for C, G, L, kind, dtype in pc.worker_gram_jobs():
            for centred in ((True, False) if kind == "exact" else (True,)):
                got = pc.run_gram_case(ops, torch, C, G, L, kind, dtype, centred)
                for name in ("gram", "tn"):
                    out[pc.key(name, C, G, L, kind, dtype, int(centred))] = got[name]
    elif what == "gemm_nt":
        for M, N, K, kind, ta, tb in pc.worker_gemm_jobs():
            for corrected in ((True, False) if kind == "exact" else (True,)):
                out[pc.key("gemm_nt", M, N, K, kind, ta, tb, int(corrected))] = pc.run_gemm_case(ops, torch, M, N, K, kind, ta, tb, corrected)
        # pitches of 16 f64 / 32 f32 genes for K = 16 / 32: whole slabs of the 128-byte shapes, half a slab of the 256-byte ones
        lib = ops._lib.lib()
        for dtype, code, K in (("float64", ops.F64, 16), ("float32", ops.F32, 32)):
            A = torch.ones((8, K), dtype=getattr(torch, dtype), device=dev)
            o = torch.full((8, 8), 7.0, dtype=torch.float64, device=dev)
            rc = lib.vcy_gemm_nt(A.data_ptr(), A.data_ptr(), None, None, 0.0, o.data_ptr(), 8, 8, K, K, K, 8, code, code, ops._stream())
            torch.cuda.synchronize()
            out[pc.key("narrow", dtype, "rc")] = np.array(rc)
            out[pc.key("narrow", dtype, "msg")] = np.frombuffer(lib.vcy_last_error() if rc else b"", dtype=np.uint8).copy()
            out[pc.key("narrow", dtype, "out")] = o.cpu().numpy()
    else:
        raise SystemExit(f"unknown job {what!r}")
    torch.cuda.synchronize()
    np.savez(out_path, **out)


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])
