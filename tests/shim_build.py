"""The build line of the tests' g++ shims (tests/*_shim.cpp: the MW_HD functions of csrc/ compiled for the host), in one place.

Strict float32: -ffp-contract=off keeps every multiply and add its own rounding, which is what the library's translation units built
without contraction compute on the device and what the bit-for-bit tests rest on.  tests/emul_build.py keeps its own lines: it caches
its builds and has a sanitizer branch."""
import ctypes as C
import subprocess

STRICT_F32 = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared"]


def strict_f32(src, path, defs=()):
    """Compiles the shim `src` to the shared object `path` (with -D for each of `defs`) and returns it loaded."""
    subprocess.run(STRICT_F32 + ["-D" + d for d in defs] + ["-o", path, src], check=True)
    return C.CDLL(path)
