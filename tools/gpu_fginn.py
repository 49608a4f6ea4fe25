"""The FGINN 2-NN (tensor_api.knn_match_fginn_batch_tensors: plain batched 2-NN + mark pass + rescan of the needy queries) against
the plain batched 2-NN (knn_match_batch_tensors) on the device.
Workload: K image pairs of 2000 x 2000 descriptors of dim 128 (64 distinct pairs repeated to K), as float32 under L2 and as uint8
under norm l2_u8.  A share of the train keypoints is twinned: a twin is one more train row 1.5 px from its original with a near-equal
descriptor, so a query whose nearest row is twinned finds the twin as its plain second neighbour and is NEEDY at spatial_th 10.
Shares of about 0 %, 10 % and 50 % of the queries; the needy share actually reached is counted on the device (slot 1 changed).
Every side runs in a child process of its own, so that the plain 2-NN can also come from another build of the library: with
--baseline-lib PATH (a libmi_degensac.so built from the parent commit) the comparison is that build on the same values; the plain
2-NN of the build under test is always measured too.  HIP events around every call after two warm-up calls; medians over --reps
calls with [min..max].
usage: gpu_fginn.py [K ...] [--reps R] [--baseline-lib PATH] [--log FILE]"""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N, DIM, BASE, R_TH = 2000, 128, 64, 10.0
SHARES = (0.0, 0.1, 0.5)


def base_pairs(share, u8):
    """(desc1 [BASE, N, DIM], desc2, kp2 [BASE, N, 2]): train rows N - t .. N - 1 are twins of rows 0 .. t - 1, t = share N / 2 (a query
    is needy when its nearest row is an original or a twin: 2 t of N rows)"""
    import numpy as np
    rng = np.random.default_rng(0)
    t = int(round(share * N / 2))
    D1, D2, K2 = [], [], []
    for _ in range(BASE):
        if u8:
            d2 = rng.integers(0, 256, (N, DIM), dtype=np.uint8)
            d2[N - t:] = d2[:t] ^ (rng.random((t, DIM)) < 0.02).astype(np.uint8)
            d1 = np.clip(d2.astype(np.int64) + rng.integers(-12, 13, d2.shape), 0, 255).astype(np.uint8)
        else:
            d2 = rng.normal(size=(N, DIM)).astype(np.float32)
            d2[N - t:] = d2[:t] + 0.002 * rng.normal(size=(t, DIM)).astype(np.float32)
            d1 = d2 + 0.15 * rng.normal(size=d2.shape).astype(np.float32)
        k2 = rng.uniform(0, 4000, (N, 2)); k2[N - t:] = k2[:t] + [1.5, 0.0]
        perm = rng.permutation(N)
        D1.append(d1[rng.permutation(N)]); D2.append(d2[perm]); K2.append(k2[perm])
    return [np.stack(x) for x in (D1, D2, K2)]


def child(side, Ks, reps):
    """one side's timings as JSON lines on stdout: {"side", "vals", "share", "K", "ms": [...], "needy", "checksum"}"""
    import torch
    from pydegensac_amd import tensor_api
    dev = torch.device("cuda", 0)
    for u8 in (False, True):
        norm = "l2_u8" if u8 else None
        for share in (SHARES if side == "fginn" else SHARES[:1]):
            bd1, bd2, bk2 = [torch.from_numpy(x).to(dev) for x in base_pairs(share, u8)]
            for K in Ks:
                rep = [(p % BASE) for p in range(K)]
                d1 = bd1[rep].reshape(K * N, DIM).contiguous(); d2 = bd2[rep].reshape(K * N, DIM).contiguous()
                k2 = bk2[rep].reshape(K * N, 2).contiguous(); c = [N] * K
                ms = []
                for r in range(reps + 2):
                    e0 = torch.cuda.Event(enable_timing=True); e1 = torch.cuda.Event(enable_timing=True)
                    e0.record()
                    if side == "fginn":
                        idx, dist = tensor_api.knn_match_fginn_batch_tensors(d1, d2, k2, c, c, R_TH, norm)
                    else:
                        idx, dist = tensor_api.knn_match_batch_tensors(d1, d2, c, c, norm=norm)
                    e1.record(); torch.cuda.synchronize()
                    if r >= 2:
                        ms.append(e0.elapsed_time(e1))
                needy = None
                if side == "fginn":
                    plain = tensor_api.knn_match_batch_tensors(d1, d2, c, c, norm=norm)[0]
                    assert bool((plain[:, 0] == idx[:, 0]).all())
                    needy = float((plain[:, 1] != idx[:, 1]).double().mean().item())
                print(json.dumps({"side": side, "vals": "u8" if u8 else "f32", "share": share, "K": K, "ms": ms, "needy": needy,
                                  "checksum": [int(idx[:, 0].to(torch.int64).sum().item()), float(dist[:, 0].double().sum().item())]}), flush=True)
                del d1, d2, k2, idx, dist
                torch.cuda.empty_cache()


def run_child(side, Ks, reps, lib):
    env = dict(os.environ)
    if lib:
        env["MI_DEGENSAC_LIB"] = os.path.abspath(lib)
    cmd = [sys.executable, os.path.abspath(__file__), "--child", side, "--reps", str(reps)] + [str(k) for k in Ks]
    out = subprocess.run(cmd, env=env, check=True, stdout=subprocess.PIPE, text=True, timeout=900).stdout
    return {(r["vals"], r["share"], r["K"]): r for r in (json.loads(ln) for ln in out.splitlines() if ln.startswith("{"))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("K", nargs="*", type=int, default=[64, 512, 2048])
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--log", default=None)
    ap.add_argument("--child", default=None)
    a = ap.parse_args()
    if a.child:
        return child(a.child, a.K, a.reps)
    import numpy as np
    lines = []

    def say(s):
        print(s, flush=True); lines.append(s)

    def fmt(v):
        return f"{np.median(v):8.3f} ms [{min(v):.3f}..{max(v):.3f}]"
    base = run_child("plain", a.K, a.reps, a.baseline_lib) if a.baseline_lib else None
    plain = run_child("plain", a.K, a.reps, None)
    fg = run_child("fginn", a.K, a.reps, None)
    say(f"# {N} x {N} x {DIM} descriptors per pair, spatial_th {R_TH}; HIP events per call, medians over {a.reps} calls [min..max] after 2 warm-up calls")
    say("# plain 2-NN baseline: " + ("a build of the parent commit (--baseline-lib), 0 % scene" if base else "the build under test (no --baseline-lib given)"))
    for vals in ("f32", "u8"):
        say(f"## {'float32 under L2' if vals == 'f32' else 'uint8 under l2_u8'}")
        for K in a.K:
            ref = (base or plain)[(vals, 0.0, K)]
            say(f"K={K:5d}  plain 2-NN baseline {fmt(ref['ms'])}" + (f"  plain 2-NN this build {fmt(plain[(vals, 0.0, K)]['ms'])}" if base else ""))
            for share in SHARES:
                r = fg[(vals, share, K)]
                add = np.median(r["ms"]) - np.median(ref["ms"])
                say(f"         FGINN, needy {100 * r['needy']:5.1f} %  {fmt(r['ms'])}  added {add:8.3f} ms = {100 * add / np.median(ref['ms']):6.1f} % of the plain 2-NN"
                    + (f"  within the baseline's [min..max]: {'yes' if np.median(r['ms']) <= max(ref['ms']) else 'NO'}" if share == 0.0 else "")
                    + (f"  slot-0 checksums equal: {'yes' if r['checksum'] == ref['checksum'] else 'NO'}" if share == 0.0 else ""))
    if a.log:
        os.makedirs(os.path.dirname(os.path.abspath(a.log)), exist_ok=True)
        with open(a.log, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
