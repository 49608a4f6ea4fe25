"""The FGINN 2-NN over a pair list (tensor_api.knn_match_fginn_pairs_tensors: descriptors and keypoints stored once per image) against
knn_match_fginn_batch_tensors on duplicated tensors (every entry's rows copied out of the stores: the path a caller had before).
Workload: a collection of M = 65 images x 2000 keypoints x dim 128 that see one scene (image i row r is a noisy copy of a common row r,
rows shuffled per image), matcher.exhaustive_pairs(65) = 2080 pairs, spatial_th 10; as float32 under L2 and as uint8 under norm l2_u8.
A share of every image's keypoints is twinned (one more row 1.5 px away with a near-equal descriptor), so a query whose nearest row is an
original or its twin is NEEDY: shares of about 0 %, 10 % and 50 %; the share reached is counted on the device (slot 1 differs from the
plain 2-NN's).
  time      every build runs in child processes of its own, alternating parent / this / parent / this; each build times --reps calls
            in all, split over its two processes, with HIP events after two warm-up calls per process; inside a process of this build
            the pair-list call and the ragged call on the duplicated tensors alternate.  Medians with [min..max].  The pair-list median and
            this build's ragged median are placed against the PARENT's ragged [min..max] on the same values (--baseline-lib: a
            libmi_degensac.so built from the parent commit, loaded through MI_DEGENSAC_LIB).
  memory    torch.cuda.max_memory_allocated (the tensors a caller holds; the library's own stream-ordered scratch is the same in both
            forms) of the pair-list call against gather + ragged call, next to the descriptor bytes the shapes give.
  identity  idx and dist bits of the pair-list call equal the ragged call's in every process of this build; checksums equal the parent's.
usage: gpu_fginn_pairs.py [--images M] [--rows N] [--reps R] [--baseline-lib FILE] [--log FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

DIM, R_TH = 128, 10.0
SHARES = (0.0, 0.1, 0.5)


def collection(m, n, share, u8):
    """(desc [m n, DIM], kps [m n, 2] float64): every image holds n rows, the last t = share n / 2 of them twins of its first t (before the
    shuffle), so 2 t of n queries meet a twinned nearest row in any other image"""
    rng = np.random.default_rng(0)
    t = int(round(share * n / 2))
    if u8:
        base = rng.integers(0, 256, (n - t, DIM), dtype=np.uint8)
    else:
        base = rng.normal(size=(n - t, DIM)).astype(np.float32)
    xy = rng.uniform(0, 4000, (n - t, 2))
    D, X = [], []
    for _ in range(m):
        if u8:
            d = np.clip(base.astype(np.int64) + rng.integers(-12, 13, base.shape), 0, 255).astype(np.uint8)
            tw = d[:t] ^ (rng.random((t, DIM)) < 0.02).astype(np.uint8)
        else:
            d = base + 0.15 * rng.normal(size=base.shape).astype(np.float32)
            tw = d[:t] + 0.002 * rng.normal(size=(t, DIM)).astype(np.float32)
        x = xy + rng.normal(size=xy.shape)
        perm = rng.permutation(n)
        D.append(np.concatenate([d, tw])[perm]); X.append(np.concatenate([x, x[:t] + [1.5, 0.0]])[perm])
    return np.concatenate(D), np.concatenate(X)


def child(a):
    """one process of one build (MI_DEGENSAC_LIB or the tree's): a JSON line per (values, share)"""
    import torch
    from pydegensac_amd import matcher, tensor_api
    dev = torch.device("cuda", 0)
    M, N = a.images, a.rows
    pairs = matcher.exhaustive_pairs(M); K = len(pairs)
    counts = [N] * M
    i_rows = torch.from_numpy((pairs[:, 0, None] * N + np.arange(N)[None]).ravel()).to(dev)
    j_rows = torch.from_numpy((pairs[:, 1, None] * N + np.arange(N)[None]).ravel()).to(dev)
    new = a.child == "this"

    def timed(fn):
        e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
        e0.record(); out = fn(); e1.record(); torch.cuda.synchronize()
        return e0.elapsed_time(e1), out

    def peak(fn):
        torch.cuda.synchronize(dev); torch.cuda.empty_cache(); torch.cuda.reset_peak_memory_stats(dev)
        base = torch.cuda.memory_allocated(dev)
        fn(); torch.cuda.synchronize(dev)
        return torch.cuda.max_memory_allocated(dev), base
    for u8 in (False, True):
        norm = "l2_u8" if u8 else None
        for share in SHARES:
            desc, kps = collection(M, N, share, u8)
            d = torch.from_numpy(desc).to(dev); k = torch.from_numpy(kps).to(dev)

            def pair_list():
                return tensor_api.knn_match_fginn_pairs_tensors(d, d, k, counts, counts, pairs, R_TH, norm)[:2]

            def ragged(t=None):
                d1, d2, k2 = t or (d[i_rows], d[j_rows], k[j_rows])
                return tensor_api.knn_match_fginn_batch_tensors(d1, d2, k2, [N] * K, [N] * K, R_TH, norm)
            out = {"vals": "u8" if u8 else "f32", "share": share}
            if new:
                out["peak_list"], out["base"] = peak(pair_list)
                out["peak_dup"], _ = peak(ragged)
            dup = (d[i_rows], d[j_rows], k[j_rows])
            for _ in range(2):
                B = ragged(dup)
                A = pair_list() if new else B
            torch.cuda.synchronize()
            out["same"] = bool(torch.equal(A[0], B[0]) and torch.equal(A[1].view(torch.int32), B[1].view(torch.int32)))
            t_list, t_rag = [], []
            for _ in range(a.reps):
                if new:
                    t_list.append(timed(pair_list)[0])
                t_rag.append(timed(lambda: ragged(dup))[0])
            out["list_ms"], out["ragged_ms"] = t_list, t_rag
            out["checksum"] = [int(B[0].to(torch.int64).sum().item()), float(B[1][:, 0].double().sum().item())]
            if new:
                plain = tensor_api.knn_match_pairs_tensors(d, d, counts, counts, pairs, norm)[0]
                out["needy"] = float((plain[:, 1] != A[0][:, 1]).double().mean().item())
                del plain
            print(json.dumps(out), flush=True)
            del dup, A, B, d, k
            torch.cuda.empty_cache()


def run_child(a, which, reps, lib):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    else:
        env.pop("MI_DEGENSAC_LIB", None)
    cmd = [sys.executable, os.path.abspath(__file__), "--images", str(a.images), "--rows", str(a.rows), "--reps", str(reps), "--child", which]
    out = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=900)
    if out.returncode != 0:
        raise RuntimeError(f"child process failed ({out.returncode}): {out.stderr[-2000:]}")
    return {(r["vals"], r["share"]): r for r in (json.loads(ln) for ln in out.stdout.splitlines() if ln.startswith("{"))}


def fmt(v):
    return f"{np.median(v):8.2f} ms [{min(v):.2f}..{max(v):.2f}]"


def side(v, ref):
    """where the median of v lies against the [min..max] of ref"""
    m = np.median(v)
    return "inside" if min(ref) <= m <= max(ref) else ("BELOW it (faster)" if m < min(ref) else "ABOVE it (slower)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=65)
    ap.add_argument("--rows", type=int, default=2000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None, help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        return child(a)
    M, N = a.images, a.rows
    K = M * (M - 1) // 2
    r1 = (a.reps + 1) // 2; r2 = max(a.reps - r1, 1)
    runs = []
    for reps in (r1, r2):
        runs.append((run_child(a, "parent", reps, a.baseline_lib) if a.baseline_lib else None, run_child(a, "this", reps, None)))
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)
    say(f"# {M} images x {N} x {DIM}, exhaustive_pairs({M}) = {K} pairs, spatial_th {R_TH}; HIP events around each call after two warm-up calls; "
        f"child processes alternate parent / this / parent / this with {r1} + {r2} = {r1 + r2} timed calls per build and form; medians [min..max]")
    say("# parent = " + ("knn_match_fginn_batch_tensors of a build of the parent commit (--baseline-lib) on the duplicated tensors" if a.baseline_lib
                          else "not measured (no --baseline-lib given)"))
    for vals in ("f32", "u8"):
        row = DIM * (4 if vals == "f32" else 1)
        say(f"## {'float32 under L2' if vals == 'f32' else 'uint8 under l2_u8'}: descriptor bytes from the shapes: stores M n row = {M * N * row / 1e6:.1f} MB, "
            f"duplicated 2 K n row = {2 * K * N * row / 1e6:.1f} MB")
        for share in SHARES:
            key = (vals, share)
            new = [r[1][key] for r in runs]
            t_list = sum((r["list_ms"] for r in new), []); t_rag = sum((r["ragged_ms"] for r in new), [])
            say(f"needy {100 * new[0]['needy']:5.1f} %  pair list {fmt(t_list)}   this build's ragged call on duplicated tensors {fmt(t_rag)}   "
                f"outputs identical (idx, dist bits): {all(r['same'] for r in new)}")
            say(f"               torch.cuda.max_memory_allocated: pair list {new[0]['peak_list'] / 1e6:9.1f} MB, duplicated (gather + call) "
                f"{new[0]['peak_dup'] / 1e6:9.1f} MB (allocated before either call, stores and row indices: {new[0]['base'] / 1e6:.1f} MB)")
            if a.baseline_lib:
                par = [r[0][key] for r in runs]
                t_par = sum((r["ragged_ms"] for r in par), [])
                ok = all(r["checksum"] == new[0]["checksum"] for r in par + new)
                say(f"               parent's ragged call {fmt(t_par)}   pair list against the parent's [min..max]: {side(t_list, t_par)} "
                    f"({100 * (np.median(t_list) / np.median(t_par) - 1):+.1f} % of its median)   this build's ragged call: {side(t_rag, t_par)} "
                    f"({100 * (np.median(t_rag) / np.median(t_par) - 1):+.1f} %)   checksums equal in every process: {ok}")
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
