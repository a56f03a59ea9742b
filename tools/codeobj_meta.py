#!/usr/bin/env python3
"""Per-kernel resources of built objects, from the code-object metadata (CPU only).

    python tools/codeobj_meta.py [--match SUBSTR]... OBJ... > meta.json
    python tools/codeobj_meta.py --compare parent.json this.json --out profiles/model_set_codeobj.json

The first form prints {kernel symbol: {vgpr, agpr, sgpr, scratch_bytes,
lds_bytes}} for the gfx950 code object of every OBJ (a hipcc .o).  The second
form puts two such dumps side by side, lists the kernels of `this` that
`parent` does not have, and exits 1 if a kernel they share differs (or a new
entry has scratch, or another LDS size than the kernel it is the twin of).
"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.path.join(os.environ.get("ROCM", "/opt/rocm"), "lib", "llvm", "bin")
FIELDS = {
    ".vgpr_count": "vgpr",
    ".agpr_count": "agpr",
    ".sgpr_count": "sgpr",
    ".private_segment_fixed_size": "scratch_bytes",
    ".group_segment_fixed_size": "lds_bytes",
}


def notes(obj, arch):
    with tempfile.TemporaryDirectory() as t:
        fat, co = os.path.join(t, "fat"), os.path.join(t, "co")
        subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", obj], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}",
                        f"--targets=hipv4-amdgcn-amd-amdhsa--{arch}", f"--output={co}"], check=True)
        return subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], check=True, capture_output=True,
                              text=True).stdout


def kernels(text):
    """The amdhsa.kernels entries of a llvm-readelf --notes dump."""
    out, cur = {}, None
    for line in text.splitlines():
        # a kernel is a list item at two spaces; its own keys sit at four (its args' deeper)
        m = re.match(r"(  - |    )(\.[a-z_]+):\s*(\S*)$", line)
        if not m:
            continue
        if m.group(1) == "  - ":
            cur = {}
        if cur is None:
            continue
        key, val = m.group(2), m.group(3).strip("'\"")
        if key in FIELDS:
            cur[FIELDS[key]] = int(val)
        elif key == ".name":
            out[val] = cur
    return {k: v for k, v in out.items() if len(v) == len(FIELDS)}


def dump(args):
    res = {}
    for obj in args.objs:
        for name, r in kernels(notes(obj, args.arch)).items():
            if not args.match or any(s in name for s in args.match):
                res[name] = r
    json.dump(res, sys.stdout, indent=1, sort_keys=True)
    print()


def kernel_of(symbol):
    """The kernel template and its arguments from a mangled symbol, without the
    parameter list: 'hf::chain::chain_rollout_kernel<..., 4>'."""
    filt = f"{LLVM}/llvm-cxxfilt" if os.path.exists(f"{LLVM}/llvm-cxxfilt") else "c++filt"
    d = subprocess.run([filt, symbol], check=True, capture_output=True, text=True).stdout.strip()
    d = re.sub(r"^void ", "", d).replace("(anonymous namespace)::", "")
    depth = 0
    for i, ch in enumerate(d):  # cut at the '(' that opens the parameter list
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            return d[:i]
    return d


def compare(args):
    """Kernels are matched by template and arguments.  A kernel of `this` whose
    last template argument is `false` where the parent has none is the parent's
    kernel behind a new defaulted parameter; its `true` twin is a new entry,
    which must have no scratch and its twin's LDS size."""
    parent, this = ({kernel_of(k): v for k, v in json.load(open(p)).items()} for p in args.compare)
    this = {(k[:-len(", false>")] + ">" if k.endswith(", false>") and k not in parent else k): v
            for k, v in this.items()}
    moved = {k: {"parent": parent[k], "this": this[k]} for k in parent if k in this and parent[k] != this[k]}
    gone = sorted(k for k in parent if k not in this)
    new = {k: this[k] for k in sorted(this) if k not in parent}
    bad_new = {}
    for k, v in new.items():
        twin = this.get(k[:-len(", true>")] + ">") if k.endswith(", true>") else None
        if v["scratch_bytes"] != 0 or (twin is not None and twin["lds_bytes"] != v["lds_bytes"]):
            bad_new[k] = v
    doc = {
        "what": "code-object metadata (gfx950) of the rollout kernels: the parent commit's build against this build; "
                "kernels keyed by template and arguments (a trailing defaulted 'false' argument dropped)",
        "existing_unchanged": not moved and not gone,
        "new_entries_scratch_free_with_their_twins_lds": not bad_new,
        "moved": moved,
        "missing_in_this": gone,
        "parent": parent,
        "this": {k: this[k] for k in sorted(parent) if k in this},
        "new": new,
    }
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"{len(parent)} existing kernels, {len(moved)} moved, {len(gone)} missing, {len(new)} new "
          f"({len(bad_new)} with scratch or another LDS size than their twin)")
    return 1 if moved or gone or bad_new else 0


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("objs", nargs="*")
    ap.add_argument("--arch", default="gfx950")
    ap.add_argument("--match", action="append", default=[])
    ap.add_argument("--compare", nargs=2, metavar=("PARENT", "THIS"))
    ap.add_argument("--out")
    a = ap.parse_args()
    sys.exit(compare(a) if a.compare else dump(a))
