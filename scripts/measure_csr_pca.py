"""Measurements of the PCA from CSR count layers on atlas.synth_atlas counts at 30 000 genes, 8 % density:
the transposition (once per fit), one projection X Z and one contraction X^T Y at l = n_components + 20 columns with the rate at
which each gathers rows of its thin operand, the per-gene moments, the number of passes and the whole fit; with --dense-at C also the
dense DevicePCA subspace pass (vcy_gemm_nt + vcy_gram_tn) on the densified f64 matrix of the same counts, the route this one complements.

    python scripts/measure_csr_pca.py --cells 200000 1000000 --dense-at 50000 --out profiles/csr_pca.txt

Times are host clocks around work that ends in a device synchronise, best of --reps after a warm-up call of the same shape."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import velocyto_amd  # noqa: E402,F401
from velocyto_amd import atlas, ops  # noqa: E402
from velocyto_amd.preprocess import DevicePCA  # noqa: E402


def best(f, reps):
    f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(time.perf_counter() - t0)
    return min(ts), max(ts)


def once(f):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = f()
    torch.cuda.synchronize()
    return r, time.perf_counter() - t0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cells", type=int, nargs="*", default=[200_000, 1_000_000])
    ap.add_argument("--genes", type=int, default=30_000)
    ap.add_argument("--density", type=float, default=0.08)
    ap.add_argument("--n-components", type=int, default=30)
    ap.add_argument("--dense-at", type=int, default=0, help="also time the dense subspace pass on the densified matrix at this many cells")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = ops.require_gpu()
    lines = []

    def say(s=""):
        print(s, flush=True)
        lines.append(s)
    G, k = a.genes, a.n_components
    say(f"# scripts/measure_csr_pca.py on {torch.cuda.get_device_name(dev)}: {G} genes, density {a.density}, n_components {k}, best (worst) of {a.reps}")
    sizes = list(a.cells) + ([a.dense_at] if a.dense_at and a.dense_at not in a.cells else [])
    for C in sizes:
        (cS, _, totS, totU, _, _), t_syn = once(lambda: atlas.synth_atlas(C, G, 4, dev, density=a.density))
        fS, _ = atlas.size_factors(totS, totU, C)
        nnz, l = cS.nnz, min(min(C, G), k + 20)
        say(f"\n## {C} cells x {G} genes: {nnz} stored elements ({100.0 * nnz / C / G:.2f} %, {cS.nbytes / 1e9:.2f} GB as CSR, "
            f"{'uint8' if cS.data.dtype == torch.uint8 else 'uint16'} counts), l = {l} columns   [generated in {t_syn:.1f} s]")
        _, t_tr = once(lambda: cS.transposed())
        op, t_tr2 = once(lambda: ops.LogNormCsr(cS, fS, 1.0))
        lens = (op.countsT.indptr[1:] - op.countsT.indptr[:-1]).double()
        say(f"transposition (gene-major copy, once per fit): {t_tr:.3f} s first call, {t_tr2:.3f} s again; elements per gene: max {int(lens.max())}, "
            f"median {int(lens.median())}, empty genes {int((lens == 0).sum())}")
        gen = torch.Generator(device=dev).manual_seed(0)
        Z = torch.linalg.qr(torch.randn((G, l), generator=gen, device=dev, dtype=torch.float64))[0]
        Y = torch.empty((C, l), dtype=torch.float64, device=dev)
        W = torch.empty((G, l), dtype=torch.float64, device=dev)
        gathered = nnz * l * 8.0                                       # bytes of thin-operand rows a product gathers
        streamed = nnz * (4 + cS.data.element_size())                  # bytes of the layer it streams
        tp, tpw = best(lambda: op.project(Z, out=Y), a.reps)
        tc, tcw = best(lambda: op.contract(Y, out=W), a.reps)
        ts, _ = best(lambda: ops.csr_lognorm_stats(op.countsT, op.scale, 1.0), a.reps)
        say(f"projection  X Z   (Z {G * l * 8 / 1e6:.0f} MB): {tp * 1e3:9.2f} ms ({tpw * 1e3:.2f})   gathers {gathered / 1e9:.1f} GB at {gathered / tp / 1e12:.2f} TB/s "
            f"(guide, 38 MB table in the Infinity Cache, 1152-B rows: 8.6 TB/s), streams the layer at {streamed / tp / 1e12:.2f} TB/s, {2.0 * nnz * l / tp / 1e12:.2f} Tflop/s")
        say(f"contraction X^T Y (Y {C * l * 8 / 1e6:.0f} MB): {tc * 1e3:9.2f} ms ({tcw * 1e3:.2f})   gathers {gathered / 1e9:.1f} GB at {gathered / tc / 1e12:.2f} TB/s "
            f"(guide, beyond the Infinity Cache, 1152-B rows: 5.5-5.8 TB/s), streams the layer at {streamed / tc / 1e12:.2f} TB/s, {2.0 * nnz * l / tc / 1e12:.2f} Tflop/s")
        say(f"moments (sum x, sum x^2 per gene): {ts * 1e3:.2f} ms ({streamed / ts / 1e12:.2f} TB/s of the layer)")
        del op, Z, Y, W
        torch.cuda.empty_cache()
        pca = DevicePCA(n_components=k)
        pcs, t_fit = once(lambda: pca.fit_transform_csr(cS, fS, 1.0))
        say(f"whole fit (transposition, moments, {pca.n_iter_} passes + Rayleigh-Ritz pass, scores): {t_fit:.3f} s, converged {pca.converged_}; "
            f"explained variance ratio of the {k} components {float(pca.explained_variance_ratio_.sum()):.4f}")
        del pcs
        if C == a.dense_at:
            X = ops.CellMatrix.empty(C, G, torch.float64)
            dense = cS.to_dense()
            for b in range(0, C, 8192):
                blk = dense.t[b:b + 8192, :G]
                blk = blk.double() if blk.dtype == torch.uint8 else (blk.to(torch.int32) & 0xFFFF).double()
                X.t[b:b + 8192, :G] = torch.log2(blk * fS[b:b + 8192, None] + 1.0)
            del dense
            mean = ops.col_means(X)
            Z = torch.linalg.qr(torch.randn((G, l), device=dev, dtype=torch.float64))[0]
            ldy = l + (l % 2)
            Yb = torch.zeros((C, ldy), dtype=torch.float64, device=dev)
            tg, _ = best(lambda: ops.gemm_nt(X, ops.CellMatrix.from_genes_major(Z, torch.float64), col_corr=(Z * mean[:, None]).sum(0), out=Yb[:, :l]), a.reps)
            tt, _ = best(lambda: ops.gram_tn(X, mean, Yb), a.reps)
            say(f"dense subspace pass on the densified f64 matrix ({C * G * 8 / 1e9:.1f} GB): projection (vcy_gemm_nt) {tg * 1e3:.2f} ms + contraction "
                f"(vcy_gram_tn) {tt * 1e3:.2f} ms = {(tg + tt) * 1e3:.2f} ms;  sparse pass above: {(tp + tc) * 1e3:.2f} ms")
            del X, Yb, Z
        del cS
        torch.cuda.empty_cache()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
