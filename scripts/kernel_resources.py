#!/usr/bin/env python3
"""VGPR / spill / scratch of every non-counting instantiation of the persistent kernel in built trace objects
(register budget check after a traversal edit; WIDE 0 binary pairs, 1 quads by entry t, 2 quads in pair order; RAW 1 =
GPU-built scenes without cold records).  usage: scripts/kernel_resources.py real-time-gpu-ray-tracer_amd/build/trace_*.o

--hash: instead, for every object given (any object that holds kernels), the sha256 (first 16 hex digits) of its gfx950
code object's .text bytes, .rodata bytes and `llvm-readelf --notes` output (kernel descriptors: registers, LDS, scratch,
arguments).  A refactor that must not change the device code compares these between a build of the parent commit and
one of the branch (profiles/refactor_*/README.md).  usage: scripts/kernel_resources.py --hash build/*.o

--hash-kernels: per kernel instead of per object, the size and sha256 of the kernel's own bytes of .text: for a change
that adds kernels to an object and must leave the others as they were (profiles/motion/README.md).

--all: registers, spills, private segment and LDS of every kernel in the objects, by demangled name (the query kernels
next to the render kernels: profiles/camera_query/kernel_resources.txt)."""
import hashlib
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def code_object(obj, d):
    """Unbundle the gfx950 code object of a host object into directory d; returns its path."""
    fb, co = f"{d}/fb", f"{d}/co"
    subprocess.run(["objcopy", "--dump-section", f".hip_fatbin={fb}", obj], check=True)
    subprocess.run([f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                    f"--input={fb}", f"--output={co}", "--unbundle"], check=True)
    return co


def notes_of(co):
    return subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True, check=True).stdout


def print_hashes(obj):
    h = lambda b: hashlib.sha256(b).hexdigest()[:16]
    with tempfile.TemporaryDirectory() as d:
        co = code_object(obj, d)
        for sec in (".text", ".rodata"):
            subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", f"--only-section={sec}", co, f"{d}/sec"], check=True)
            with open(f"{d}/sec", "rb") as f:
                print(f"{obj.split('/')[-1]} {sec} {h(f.read())}")
        print(f"{obj.split('/')[-1]} notes {h(notes_of(co).encode())}")


def print_kernel_hashes(obj):
    """Per kernel of the object, by demangled name: the size and sha256 (first 16 hex digits) of its own bytes of .text."""
    h = lambda b: hashlib.sha256(b).hexdigest()[:16]
    with tempfile.TemporaryDirectory() as d:
        co = code_object(obj, d)
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.text", co, f"{d}/sec"], check=True)
        with open(f"{d}/sec", "rb") as f:
            text = f.read()
        sections = subprocess.run([f"{LLVM}/llvm-readelf", "-S", "-W", co], capture_output=True, text=True, check=True).stdout
        base = int(re.search(r"\s\.text\s+PROGBITS\s+([0-9a-f]+)", sections).group(1), 16)
        symbols = subprocess.run([f"{LLVM}/llvm-readelf", "-s", "-W", co], capture_output=True, text=True, check=True).stdout
    rows = []
    for line in symbols.splitlines():
        m = re.match(r"\s*\d+:\s+([0-9a-f]+)\s+(\d+)\s+FUNC\s+\S+\s+\S+\s+\S+\s+(\S+)", line)
        if m:
            at, size = int(m.group(1), 16) - base, int(m.group(2))
            dem = subprocess.run(["c++filt", m.group(3)], capture_output=True, text=True).stdout.strip()
            dem = re.sub(r"\(.*", "", dem.replace("(anonymous namespace)::", "")).replace("void ", "")
            rows.append(f"{obj.split('/')[-1]} {dem} {size} {h(text[at:at + size])}")
    print("\n".join(sorted(set(rows))))                      # a kernel is in .dynsym and in .symtab


def print_resources(obj):
    with tempfile.TemporaryDirectory() as d:
        notes = notes_of(code_object(obj, d))
    for e in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        m = re.search(r"render_persistent_kernelILb([01])ELi(\d)ELi(\d)ELi(\d)E", name)
        if not m or m.group(1) != "0":
            continue
        label = f"WPE {m.group(2)} WIDE {m.group(3)} RAW {m.group(4)}"
        g = lambda k: re.search(rf"\.{k}:\s+(\d+)", e).group(1)
        print(f"{obj.split('/')[-1]:22s} {label:22s} vgpr {g('vgpr_count'):>3} vspill {g('vgpr_spill_count'):>3} "
              f"sgpr {g('sgpr_count'):>3} sspill {g('sgpr_spill_count'):>3} scratch {g('private_segment_fixed_size')}")


def print_all(obj):
    """Every kernel of the object, by demangled name: registers, spills, private segment, LDS."""
    with tempfile.TemporaryDirectory() as d:
        notes = notes_of(code_object(obj, d))
    rows = []
    for e in notes.split("- .agpr_count")[1:]:
        name = re.search(r"\.name:\s+(\S+)", e).group(1)
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"rtamd::dev_\w+::", "", dem).replace("(anonymous namespace)::", "")
        dem = re.sub(r"\(.*", "", dem).replace("void ", "")
        g = lambda k: re.search(rf"\.{k}:\s+(\d+)", e).group(1)
        rows.append(f"{obj.split('/')[-1]:18s} {dem:46s} vgpr {g('vgpr_count'):>3} vspill {g('vgpr_spill_count'):>3} "
                    f"sgpr {g('sgpr_count'):>3} sspill {g('sgpr_spill_count'):>3} scratch {g('private_segment_fixed_size'):>4} "
                    f"lds {g('group_segment_fixed_size'):>6}")
    print("\n".join(sorted(rows)))


if __name__ == "__main__":
    args = sys.argv[1:]
    mode = print_hashes if "--hash" in args else (print_all if "--all" in args else print_resources)
    if "--hash-kernels" in args:
        mode = print_kernel_hashes
    for obj in (a for a in args if a not in ("--hash", "--all", "--hash-kernels")):
        mode(obj)
