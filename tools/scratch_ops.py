"""CPU only: per-function scratch and FLAT instruction counts of a device assembly listing (`hipcc --cuda-device-only -S`).
usage: hipcc <FLAGS of the Makefile> --cuda-device-only -S pydegensac_amd/csrc/mi_degensac_t256.hip -o /tmp/t256.s
       python tools/scratch_ops.py /tmp/t256.s [name-filter ...]
Columns: scratch stores, scratch loads, FLAT stores, FLAT loads (static counts), then the demangled function name.
tests/test_lo_scratch_ops.py imports functions() from here."""
import re
import subprocess
import sys

_FN = re.compile(r"^\s*\.type\s+([^,\s]+),@function")


def functions(asm_text):
    """{mangled name: {"scratch_store", "scratch_load", "flat_store", "flat_load": static counts}} of every function in the listing"""
    out, cur = {}, None
    for line in asm_text.splitlines():
        m = _FN.match(line)
        if m:
            cur = out.setdefault(m.group(1), {"scratch_store": 0, "scratch_load": 0, "flat_store": 0, "flat_load": 0})
            continue
        if cur is None:
            continue
        s = line.lstrip()
        if s.startswith(".Lfunc_end"):
            cur = None
        elif s.startswith("scratch_store"):
            cur["scratch_store"] += 1
        elif s.startswith("scratch_load"):
            cur["scratch_load"] += 1
        elif s.startswith("flat_store") or s.startswith("flat_atomic"):
            cur["flat_store"] += 1
        elif s.startswith("flat_load"):
            cur["flat_load"] += 1
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return r.stdout.splitlines()
    except (OSError, subprocess.CalledProcessError):
        return list(names)


if __name__ == "__main__":
    fns = functions(open(sys.argv[1]).read())
    names = sorted(fns, key=lambda k: -(fns[k]["scratch_store"] + fns[k]["scratch_load"]))
    filt = sys.argv[2:]
    print("# %s: static counts per function" % sys.argv[1].split("/")[-1])
    print("%6s %6s %6s %6s  %s" % ("sc_st", "sc_ld", "fl_st", "fl_ld", "function"))
    for k, d in zip(names, demangle(names)):
        if filt and not any(f in d for f in filt):
            continue
        c = fns[k]
        print("%6d %6d %6d %6d  %s" % (c["scratch_store"], c["scratch_load"], c["flat_store"], c["flat_load"], d.split("(")[0]))
