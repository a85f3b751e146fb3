"""Builds and runs tools/launch_plan_dump.cpp: what csrc/launch_plan.h plans for a grid of configurations, as a stand-alone host program
with AddressSanitizer and UndefinedBehaviorSanitizer — no device, no launch, no Python in the process.  engine.hip and the tool are
compiled for the wavefront emulator (tools/hipemu) with -fsanitize=address,undefined; the rest of the library is linked from the
emulator's plain objects (tools/hipemu/build_emu.py).  Developer tool, and what tests/test_launch_plan.py runs.

    python tools/launch_plan_dump.py [out.txt]     the lines go to out.txt (default: stdout); exits with the program's status
                                                   (0: the grid covers both tables, the packed rows exclude each other, no sanitizer report)
    python tools/launch_plan_dump.py --record      rewrites tests/golden/launch_plan.txt.xz (with a deliberate layout change, in its commit)"""
import lzma
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
import build_emu as B   # noqa: E402

SANITIZED = ["engine.hip"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1"]
# the sanitizer runtimes are linked into the program: it then starts whatever else the environment has the loader bring in first
LINK_SAN = ["-static-libasan", "-static-libubsan"]
GOLDEN = os.path.join(ROOT, "tests", "golden", "launch_plan.txt.xz")


def build():
    from maelstrom_amd.build import SOURCES
    B.build()
    out = os.path.join(B.OBJ, "asan")
    os.makedirs(out, exist_ok=True)
    objs = []
    for s in SOURCES:
        obj = os.path.join(B.OBJ, s + ".o")
        if s in SANITIZED:
            obj = os.path.join(out, s + ".o")
            subprocess.run([B.CXX] + B.FLAGS + SAN + ["-x", "c++", "-c", "-o", obj, os.path.join(B.CSRC, s)], check=True)
        objs.append(obj)
    exe = os.path.join(out, "launch_plan_dump")
    subprocess.run([B.CXX] + B.FLAGS + SAN + LINK_SAN + ["-o", exe, os.path.join(ROOT, "tools", "launch_plan_dump.cpp")] + objs + [os.path.join(B.OBJ, "hipemu.cpp.o"), "-ldl", "-pthread"], check=True)
    return exe


def run(exe):
    """(exit status, the program's lines as bytes)"""
    env = dict(os.environ, ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("MSIM_DEV_FLAGS", "MSIM_POISON", "MSIM_GUARD"):
        env.pop(k, None)
    r = subprocess.run([exe], env=env, stdout=subprocess.PIPE)
    return r.returncode, r.stdout


def main():
    rc, lines = run(build())
    if "--record" in sys.argv:
        if rc == 0:
            with lzma.open(GOLDEN, "wb", preset=9 | lzma.PRESET_EXTREME) as f:
                f.write(lines)
    elif len(sys.argv) > 1:
        with open(sys.argv[1], "wb") as f:
            f.write(lines)
    else:
        sys.stdout.buffer.write(lines)
    return rc


if __name__ == "__main__":
    sys.exit(main())
