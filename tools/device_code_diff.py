"""Is the device code of two builds the same?  usage: python tools/device_code_diff.py OLD_OBJ_DIR NEW_OBJ_DIR

Both directories hold the objects of audio_diffusion_pytorch_amd/build.py (<source>.hip.o).  For every translation unit the gfx950
code object is unbundled and compared per kernel symbol: the set of symbols, each kernel's disassembly and its resource figures
(VGPR / SGPR / LDS / scratch / ... of the code object's metadata).  Runs without a GPU.  Exit status 1 on any difference."""
import glob
import os
import re
import shutil
import subprocess
import sys
import tempfile

LLVM = os.environ.get("ROCM_LLVM", "/opt/rocm/lib/llvm/bin")


def code_object(obj, tmp):
    """the gfx950 code object embedded in a host object (llvm-objdump --offloading writes it next to its input)"""
    sub = tempfile.mkdtemp(dir=tmp)
    copy = shutil.copy(obj, sub)
    subprocess.check_call([os.path.join(LLVM, "llvm-objdump"), "--offloading", copy], stdout=subprocess.DEVNULL)
    (co,) = glob.glob(copy + ".*gfx950")
    return co


def kernels(co):
    """{symbol: (disassembly without addresses, metadata block)}"""
    dis = subprocess.check_output([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", "--no-leading-addr", co], text=True)
    body, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"^<(.+)>:$", line.strip())
        if m:
            cur = m.group(1)
            body[cur] = []
        elif cur is not None:
            body[cur].append(re.sub(r"\s*//.*$", "", line))  # (the trailing comment is the instruction's address)
    notes = subprocess.check_output([os.path.join(LLVM, "llvm-readelf"), "--notes", co], text=True)
    meta = {}
    for block in re.split(r"\n\s*- (?=\.agpr_count|\.args)", notes):
        m = re.search(r"\.name:\s+(\S+)", block)
        if m:
            meta[m.group(1)] = "\n".join(l.strip() for l in block.splitlines() if re.search(
                r"\.(agpr_count|vgpr_count|sgpr_count|group_segment_fixed_size|private_segment_fixed_size|kernarg_segment_size|"
                r"max_flat_workgroup_size|sgpr_spill_count|vgpr_spill_count|wavefront_size|uses_dynamic_stack):", l))
    for v in body.values():  # (alignment padding between symbols, shown as '...', and the s_code_end padding the last symbol of the section owns)
        while v and (not v[-1].strip() or v[-1].split()[0] in ("s_code_end", "s_nop", "...")):
            v.pop()
    return {k: ("\n".join(v), meta.get(k, "")) for k, v in body.items()}


def main():
    old_dir, new_dir = sys.argv[1:3]
    bad = total = 0
    with tempfile.TemporaryDirectory() as tmp:
        names = sorted({os.path.basename(p) for d in (old_dir, new_dir) for p in glob.glob(os.path.join(d, "*.hip.o"))})
        for n in names:
            a, b = (kernels(code_object(os.path.join(d, n), tmp)) for d in (old_dir, new_dir))
            total += len(b)
            for k in sorted(set(a) | set(b)):
                if a.get(k) != b.get(k):
                    bad += 1
                    what = "only in one build" if k not in a or k not in b else ("code" if a[k][0] != b[k][0] else "resources")
                    print(f"{n}: {k}: {what} differ")
    print(f"{len(names)} translation units, {total} device symbols, {bad} differences")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
