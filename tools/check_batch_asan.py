"""Builds and runs tools/check_batch_asan.cpp: the batch entries of the device checkers as a stand-alone host program with
AddressSanitizer, LeakSanitizer and UndefinedBehaviorSanitizer — no device, no Python in the process.  The checker units, the host
checkers behind them and the allocator are compiled for the wavefront emulator (tools/hipemu) with -fsanitize=address,undefined; the
rest of the library is linked from the emulator's plain objects (tools/hipemu/build_emu.py).  Developer tool.

    python tools/check_batch_asan.py        exits with the program's status (0: every entry MSIM_OK, no sanitizer report)"""
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools", "hipemu"))
import build_emu as B   # noqa: E402

SANITIZED = ["checker.hip", "set_check.cpp", "lin_check_dev.hip", "txn_check_dev.hip", "rw_check_dev.hip", "kafka_check_dev.hip", "pn_check_dev.hip", "unique_check_dev.hip", "perf_check_dev.hip",
             "lin_check.cpp", "txn_check.cpp", "kafka_check.cpp", "pn_check.cpp", "guard.cpp"]
SAN = ["-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-O1"]


def main():
    from maelstrom_amd.build import SOURCES
    B.build()
    out = os.path.join(B.OBJ, "asan")
    os.makedirs(out, exist_ok=True)
    objs = []
    for s in SOURCES:
        if s in SANITIZED:
            obj = os.path.join(out, s + ".o")
            subprocess.run([B.CXX] + B.FLAGS + SAN + ["-x", "c++", "-c", "-o", obj, os.path.join(B.CSRC, s)], check=True)
        else:
            obj = os.path.join(B.OBJ, s + ".o")
        objs.append(obj)
    exe = os.path.join(out, "check_batch_asan")
    subprocess.run([B.CXX] + B.FLAGS + SAN + ["-o", exe, os.path.join(ROOT, "tools", "check_batch_asan.cpp")] + objs + [os.path.join(B.OBJ, "hipemu.cpp.o"), "-ldl", "-pthread"], check=True)
    env = dict(os.environ, HIPEMU_DIVERGENT="1", ASAN_OPTIONS="detect_leaks=1", UBSAN_OPTIONS="print_stacktrace=1")
    for k in ("LD_PRELOAD", "MSIM_DEV_FLAGS", "MSIM_POISON", "MSIM_GUARD"):
        env.pop(k, None)
    return subprocess.run([exe], env=env).returncode


if __name__ == "__main__":
    sys.exit(main())
