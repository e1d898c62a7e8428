#!/usr/bin/env python3
"""Compare the gfx950 kernels of two builds, symbol by symbol: tools/codeobj_diff.py A B, each a librmc.so or
an rmc_kernels.o.  Per kernel whose bytes or resources differ: size, VGPRs (.vgpr_count: the unified file,
AGPRs included), AGPRs, SGPRs, scratch, LDS and the waves per SIMD the registers allow (512 per lane in
granules of 8, 8 waves at most); then a summary per kernel family.  Bytes and metadata only: no instruction
is looked at.  Exit status 1 if a kernel of A is missing in B or one's scratch, LDS, SGPRs or waves per SIMD
got worse."""
import collections, os, re, subprocess, sys, tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"
FIELDS = ("vgpr_count", "agpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def tool(name, *args):
    return subprocess.check_output([os.path.join(LLVM, name), *args], text=True)


def code_objects(path, tmp):
    """the gfx950 ELFs of every offload bundle in the file (one bundle per translation unit)"""
    data = open(path, "rb").read()
    starts = [m.start() for m in re.finditer(MAGIC, data)]
    for i, (a, b) in enumerate(zip(starts, starts[1:] + [len(data)])):
        blob, elf = os.path.join(tmp, f"{i}.hipfb"), os.path.join(tmp, f"{i}.elf")
        open(blob, "wb").write(data[a:b])
        tool("clang-offload-bundler", "--unbundle", "--type=o", "--allow-missing-bundles", f"--input={blob}",
             "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={elf}")
        if os.path.getsize(elf):
            yield elf


def kernels(path):
    """symbol -> (code bytes, metadata tuple in FIELDS' order)"""
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for elf in code_objects(path, tmp):
            meta = {}
            for k in re.split(r"\n\s+- \.agpr_count", tool("llvm-readelf", "--notes", elf))[1:]:
                k = ".agpr_count" + k
                meta[re.search(r"\.name:\s+(\S+)", k).group(1)] = tuple(
                    int(re.search(r"\." + f + r":\s+(\d+)", k).group(1)) for f in FIELDS)
            sec = {}  # section index -> (address, file offset)
            for m in re.finditer(r"\[\s*(\d+)\]\s+\S+\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s", tool("llvm-readelf", "--sections", "--wide", elf)):
                sec[m.group(1)] = (int(m.group(2), 16), int(m.group(3), 16))
            data = open(elf, "rb").read()
            for line in tool("llvm-readelf", "--symbols", "--wide", elf).splitlines():
                p = line.split()
                if len(p) >= 8 and p[3] == "FUNC" and p[7] in meta and p[6] in sec:
                    addr, off = sec[p[6]]
                    at = off + int(p[1], 16) - addr
                    out[p[7]] = (data[at:at + int(p[2])], meta[p[7]])
    return out


def waves(m):
    return min(8, 512 // max(8, (m[0] + 7) // 8 * 8))


def family(sym):
    m = re.search(r"\d+(k_[a-z_0-9]+?)I", sym) or re.search(r"\d+(k_[a-z_0-9]+)", sym)
    return m.group(1) if m else sym


def main(a_path, b_path):
    A, B = kernels(a_path), kernels(b_path)
    fam = collections.defaultdict(lambda: collections.Counter())
    worse = 0
    print(f"A = {a_path}: {len(A)} kernels; B = {b_path}: {len(B)} kernels")
    print("per kernel that differs: bytes | size vgpr agpr sgpr scratch lds waves/SIMD (A -> B)")
    for sym in sorted(A):
        f = fam[family(sym)]
        f["n"] += 1
        if sym not in B:
            f["missing"] += 1
            worse += 1
            print(f"MISSING in B  {sym}")
            continue
        (ca, ma), (cb, mb) = A[sym], B[sym]
        same = ca == cb
        f["identical" if same else "same size+meta" if (len(ca), ma) == (len(cb), mb) else "changed"] += 1
        bad = mb[2:] != ma[2:] or waves(mb) < waves(ma)
        f["worse"] += bad
        worse += bad
        if not same and ((len(ca), ma) != (len(cb), mb) or "-v" in sys.argv):
            print(f"{'WORSE' if bad else 'differs'}  {sym}\n    {len(ca)} {' '.join(map(str, ma))} {waves(ma)} -> "
                  f"{len(cb)} {' '.join(map(str, mb))} {waves(mb)}"
                  + (f"  ({sum(x != y for x, y in zip(ca, cb))} bytes differ)" if len(ca) == len(cb) else ""))
    print("per family: kernels, byte-identical, same size and metadata (bytes differ), changed, resources worse, missing")
    for name, f in sorted(fam.items()):
        print(f"  {name:18s} {f['n']:4d} {f['identical']:4d} {f['same size+meta']:4d} {f['changed']:4d} {f['worse']:4d} {f['missing']:4d}")
    print(f"new in B: {len(set(B) - set(A))}; resources worse or missing: {worse}")
    return 1 if worse else 0


if __name__ == "__main__":
    paths = [a for a in sys.argv[1:] if not a.startswith("-")]
    if len(paths) != 2:
        sys.exit(__doc__)
    sys.exit(main(*paths))
