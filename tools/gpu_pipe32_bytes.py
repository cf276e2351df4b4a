"""Same bytes from two builds of the library: SHA-256 of everything the 32-row attention kernel (csrc/shared_attn_fwd_pipe.hip)
writes - ``out``, ``lse`` and, on the forms that carry it, ``seg_mass`` - over every product form, both dtypes, with and without the
AdaIN affine, on three small shapes that reach every branch of the kernel: single ragged tiles with a partial last query block
(shape 1), the steady-state pair loop with both tails (shape 2, twelve tiles), an odd tile count without a self block (shape 3).

    kind        tuning values
    plain       7, 10, 11, 14, 18 (refused without pre-scaled Q: listed as such), 0
    presc       11, 18, 0          IR_FLAG_Q_PRESCALED
    valid       11, 14             valid_refs: a zero-filled suffix of the reference list
    bias        0, 11, 14          key bias with masked keys and one fully masked reference
    counts      0, 11, 14          ref_lens, two count sets per shape: counts of 0, of 1 and full counts among them

Every case runs as planned and with ``IR_ATTN_FORCE_SPLIT=3`` (every item cut into three K/V-range pieces: the piece epilogue,
the workspace, both combine kernels, pieces that end mid-segment).  That variable is read once per process, so each build runs in
two worker processes, one after the other; this process never opens the GPU.  A worker that fails ends the run.

usage: python tools/gpu_pipe32_bytes.py --parent-lib PATH/libinstantrestore_hip.so [--out FILE]
The two listings must be identical; exit status 1 when they are not."""
import argparse
import hashlib
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = (("1", 2, 2, 72, 3, 40, True), ("2", 1, 3, 200, 2, 200, True), ("3", 1, 3, 200, 2, 200, False))   # name, B, H, L, N, Lr, self
KINDS = (("plain", (7, 10, 11, 14, 18, 0)), ("presc", (11, 18, 0)), ("valid", (11, 14)), ("bias", (0, 11, 14)), ("counts", (0, 11, 14)))
MASS_TUNINGS = (0, 11, 14)     # the forms that carry seg_mass
SCALE = 0.125


def sha(t):
    import torch
    return hashlib.sha256(t.detach().cpu().contiguous().view(-1).view(torch.uint8).numpy().tobytes()).hexdigest()[:32]


def worker():
    import torch
    sys.path.insert(0, REPO)
    from instantrestore_amd import _lib, ops
    dev = torch.device("cuda:0")
    split = os.environ.get("IR_ATTN_FORCE_SPLIT", "-")
    for name, B, H, L, N, Lr, inc in SHAPES:
        for dtype in (torch.float16, torch.bfloat16):
            g = torch.Generator().manual_seed(1000 + len(name) + B * 7 + L)
            rnd = lambda *s: torch.randn(*s, generator=g)
            q, k, v = (rnd(B, L, H * 64).to(dtype).to(dev) for _ in range(3))
            rk, rv = rnd(B, N, Lr, H * 64).to(dtype).to(dev), (rnd(B, N, Lr, H * 64) * 1.5 + 0.3).to(dtype).to(dev)
            qs = (q.float() * (SCALE * 1.4426950408889634)).to(dtype)
            lkv = (L if inc else 0) + N * Lr
            bias = rnd(B, lkv) * 0.5
            bias[torch.rand(B, lkv, generator=g) < 0.1] = float("-inf")
            r1 = (L if inc else 0) + Lr
            bias[:, r1:r1 + Lr] = float("-inf")                              # reference 1: every key masked
            bias = bias.to(dev)
            valid = torch.tensor([1, 2][:B], dtype=torch.int32, device=dev)
            rkz, rvz = rk.clone(), rv.clone()
            for b in range(B):
                rkz[b, int(valid[b]):] = 0
                rvz[b, int(valid[b]):] = 0
            counts = {"1": ([[0, 1, 40], [40, 17, 0]], [[40, 40, 40], [1, 0, 33]])}.get(name, ([[0, 200]], [[1, 137]]))
            for adain in (False, True):
                for kind, tunings in KINDS:
                    variants = [("", {})]
                    refs = (rk, rv)
                    if kind == "presc":
                        variants = [("", {"q_prescaled": True})]
                    elif kind == "valid":
                        variants, refs = [("", {"valid_refs": valid})], (rkz, rvz)
                    elif kind == "bias":
                        variants = [("", {"key_bias": bias})]
                    elif kind == "counts":
                        variants = [(f" set{i}", {"ref_lens": torch.tensor(c, dtype=torch.int32, device=dev)}) for i, c in enumerate(counts)]
                    aff = ops.adain_stats(v, refs[1], heads=H) if adain else None
                    for tuning in tunings:
                        for tag, extra in variants:
                            for mass in ((False, True) if tuning in MASS_TUNINGS else (False,)):
                                head = f"shape {name} {str(dtype)[6:]:8s} adain {int(adain)} {kind:6s}{tag} tuning {tuning:2d} mass {int(mass)} split {split}:"
                                prev = ops.set_attn_variant(tuning)
                                try:
                                    res = ops.shared_attention(qs if kind == "presc" else q, k, v, refs[0], refs[1], heads=H, scale=SCALE, include_self=inc,
                                                               adain=aff, return_lse=True, return_mass=mass, **extra)
                                    torch.cuda.synchronize()
                                except (_lib.IRError, ValueError) as e:
                                    # a refusal by the argument check (status -1 / -2, or ops' own: no launch happened) is part of the listing
                                    if isinstance(e, _lib.IRError) and "status -1:" not in str(e) and "status -2:" not in str(e):
                                        raise
                                    print(head, "refused:", str(e).splitlines()[0][:110], flush=True)
                                    continue
                                finally:
                                    ops.set_attn_variant(prev)
                                print(head, " ".join(sha(t) for t in res), flush=True)


def digest_table(new, old):
    """one row per (shape, kind, split): lines, SHA-256 of each build's lines of the group - the listings in a form that fits a profile"""
    groups = {}
    for which, lines in (("new", new), ("old", old)):
        for l in lines:
            f = l.split()
            key = (f[1], f[5], l.split(" split ")[1].split(":")[0])
            groups.setdefault(key, {"new": [], "old": []})[which].append(l)
    rows = ["# shape kind   split | lines new / parent | digest new | digest parent | same?"]
    for (shape, kind, split), g in groups.items():
        d = {w: hashlib.sha256("\n".join(g[w]).encode()).hexdigest()[:16] for w in g}
        rows.append(f"  {shape:5s} {kind:6s} {split:5s} | {len(g['new']):4d} / {len(g['old']):4d} | {d['new']} | {d['old']} | {'=' if g['new'] == g['old'] else 'DIFFERENT'}")
    return rows


def run_build(lib, limit):
    lines = []
    for split in (None, "3"):
        env = dict(os.environ)
        env.pop("IR_ATTN_FORCE_SPLIT", None)
        env.pop("IR_LIB_PATH", None)
        if split:
            env["IR_ATTN_FORCE_SPLIT"] = split
        if lib:
            env["IR_LIB_PATH"] = os.path.abspath(lib)
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--worker"], env=env, capture_output=True, text=True, timeout=limit)
        if r.returncode != 0:
            sys.stderr.write(r.stdout[-2000:] + r.stderr[-4000:])
            raise SystemExit(f"worker ({lib or 'this build'}, split {split}) ended with status {r.returncode}: nothing more is run")
        lines += [l for l in r.stdout.splitlines() if l.startswith("shape ")]
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", required=False)
    ap.add_argument("--out")
    ap.add_argument("--limit", type=int, default=240, help="seconds per worker process")
    ap.add_argument("--worker", action="store_true")
    a = ap.parse_args()
    if a.worker:
        return worker()
    new = run_build(None, a.limit)
    text = [f"# this build: {len(new)} lines"] + new
    same = True
    if a.parent_lib:
        old = run_build(a.parent_lib, a.limit)
        same = old == new
        text += [f"# parent build ({a.parent_lib}): {len(old)} lines"] + old
        text += digest_table(new, old)
        text += [f"# the two listings are {'IDENTICAL' if same else 'DIFFERENT'}: {len(new)} / {len(old)} lines, "
                 f"{sum(1 for x, y in zip(new, old) if x != y) + abs(len(new) - len(old))} differ"]
    out = "\n".join(text) + "\n"
    sys.stdout.write(out)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(out)
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
