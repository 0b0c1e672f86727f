#!/usr/bin/env python3
"""Checksums of the gfx950 device code of built objects: tools/device_code.py [-k] [build dir, default scaleprotoseg_amd/csrc/build]
One line per translation unit: sha1 of the code object's .text, its size, the number of kernel descriptors (*.kd) and a
digest of the sorted per-kernel checksums (equal when only the ORDER of the kernels in .text differs).  -k adds one line
per kernel: checksum of its bytes and its (mangled) name.  Two builds of one source differ in the .o and the code object
(a per-compilation symbol) but not in .text, so these lines are what to diff when a kernel source was only tidied.
Registers, scratch, LDS and occupancy per kernel: tools/kernel_regs.sh."""
import glob, hashlib, os, subprocess, sys, tempfile

BIN = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin")
run = lambda *c: subprocess.run([os.path.join(BIN, c[0]), *c[1:]], check=True, capture_output=True, text=True).stdout
sha = lambda b: hashlib.sha1(b).hexdigest()[:16]
args = [a for a in sys.argv[1:] if a != "-k"]
build = args[0] if args else os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "scaleprotoseg_amd", "csrc", "build")
for obj in sorted(glob.glob(os.path.join(build, "*.o"))):
    with tempfile.TemporaryDirectory() as d:
        fb, co, tx = (os.path.join(d, n) for n in ("fatbin", "co", "text"))
        try:
            run("llvm-objcopy", "--dump-section", ".hip_fatbin=" + fb, obj)
        except subprocess.CalledProcessError:
            print("%-14s no device code" % os.path.basename(obj)[:-2])
            continue
        run("clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb, "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co)
        run("llvm-objcopy", "-O", "binary", "--only-section=.text", co, tx)
        text = open(tx, "rb").read()
        base = next(int(l.split()[l.split().index(".text") + 2], 16) for l in run("llvm-readelf", "-SW", co).splitlines() if " .text " in l)
        syms = [l.split() for l in run("llvm-readelf", "-sW", co).splitlines()]
        kds = {s[7] for s in syms if len(s) == 8 and s[7].endswith(".kd")}
        kern = sorted((sha(text[int(s[1], 16) - base:int(s[1], 16) - base + int(s[2])]), s[7]) for s in syms
                      if len(s) == 8 and s[3] == "FUNC" and s[7] + ".kd" in kds)
    print("%-14s text=%s bytes=%d kd=%d kernels=%s" % (os.path.basename(obj)[:-2], sha(text), len(text), len(kds), sha("".join(k for k, _ in kern).encode())))
    if "-k" in sys.argv:
        for k, name in kern:
            print("   ", k, name)
