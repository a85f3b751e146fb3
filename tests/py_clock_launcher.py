"""Runs an UNMODIFIED Python Maelstrom node program (e.g. the reference's demo/python/broadcast.py) in virtual time, for replays:

    python tests/py_clock_launcher.py <program.py> [args...]

  * `asyncio.timeout` (3.11) is provided for older interpreters: a deadline on the running loop's clock that cancels the task and turns
    the cancellation into TimeoutError, as the 3.11 context manager does;
  * the event loop's clock is virtual: loop.time() is the last value the harness set, so timers (the 1 s RPC timeouts) fire only when
    the harness moves the clock;
  * the harness moves it with a control line {"__clock__": <microseconds>} on stdin.  The program never sees that line: stdin is wrapped,
    and the wrapper (running in the program's reader thread) sets the clock and wakes the loop, which then runs whatever became due.

Everything else — stdin / stdout / stderr, the program's own threads — is untouched.  Test infrastructure only."""
import asyncio
import json
import os
import runpy
import sys

_now_us = [0]
_loops = []


class _Timeout:
    """asyncio.timeout(delay) for interpreters without it"""

    def __init__(self, delay):
        self.delay, self.expired, self.handle, self.task = delay, False, None, None

    def _fire(self):
        self.expired = True
        self.task.cancel()

    async def __aenter__(self):
        loop = asyncio.get_running_loop()
        self.task = asyncio.current_task()
        if self.delay is not None:
            self.handle = loop.call_at(loop.time() + self.delay, self._fire)
        return self

    async def __aexit__(self, et, e, tb):
        if self.handle is not None:
            self.handle.cancel()
        if self.expired and et is asyncio.CancelledError:
            raise TimeoutError
        return False


class _VirtualClockPolicy(asyncio.DefaultEventLoopPolicy):
    def new_event_loop(self):
        loop = super().new_event_loop()
        loop.time = lambda: _now_us[0] / 1e6
        _loops.append(loop)
        return loop


class _Stdin:
    """sys.stdin for the program: control lines set the clock and are swallowed"""

    def __init__(self, f):
        self.f = f

    def readline(self):
        while True:
            line = self.f.readline()
            if line.startswith('{"__clock__"'):
                _now_us[0] = int(json.loads(line)["__clock__"])
                for loop in _loops:
                    if not loop.is_closed():
                        loop.call_soon_threadsafe(lambda: None)   # wake the selector: due timers run now
                continue
            return line

    def __getattr__(self, name):
        return getattr(self.f, name)


def main():
    prog = os.path.abspath(sys.argv[1])
    if not hasattr(asyncio, "timeout"):
        asyncio.timeout = _Timeout
    asyncio.set_event_loop_policy(_VirtualClockPolicy())
    sys.stdin = _Stdin(sys.stdin)
    sys.argv = sys.argv[1:]
    sys.path[0] = os.path.dirname(prog)
    runpy.run_path(prog, run_name="__main__")


if __name__ == "__main__":
    main()
