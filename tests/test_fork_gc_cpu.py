"""CPU: a process forked after `import ppt_amd` never runs the cyclic collector over what it inherited (ppt_amd/__init__.py): a
garbage cycle of the parent stays unfinalised in the child, while the child's own cycles are still collected."""
import gc
import os

import pytest


class _Finalised:
    def __init__(self, fd, tag):
        self.fd, self.tag = fd, tag
        self.me = self                                       # a reference cycle: only the cyclic collector frees it

    def __del__(self):
        os.write(self.fd, self.tag)


@pytest.mark.skipif(not hasattr(os, "fork"), reason="needs fork")
def test_forked_child_does_not_collect_the_inherited_heap():
    import ppt_amd  # noqa: F401
    r, w = os.pipe()
    was_on = gc.isenabled()
    gc.disable()                                             # the parent must not collect the cycle before the fork
    try:
        _Finalised(w, b"P")                                  # garbage cycle, left for the collector
        pid = os.fork()
        if pid == 0:                                         # child: a full collection, then one cycle of its own
            try:
                gc.enable()
                gc.collect()
                _Finalised(w, b"C")
                gc.collect()
            finally:
                os._exit(0)
        _, status = os.waitpid(pid, 0)
        gc.collect()                                         # the parent finalises its own cycle: "P" after the child's "C"
        os.close(w)
        out = b""
        while True:
            chunk = os.read(r, 64)
            if not chunk:
                break
            out += chunk
        os.close(r)
    finally:
        if was_on:
            gc.enable()
    assert os.WIFEXITED(status) and os.WEXITSTATUS(status) == 0
    assert out == b"CP", out
