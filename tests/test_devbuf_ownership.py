"""Who frees what (mina_bridge_amd/csrc/ctx.h): DevBuf and PinnedBuf free themselves, a borrowed DevBuf never frees its parent's block, and a Lane, an SrsState, a
mina_ctx and a view's Installed leave nothing behind when they go -- without a list of their buffers anywhere."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUZZ = os.path.join(ROOT, "tests", "fuzz")


def test_buffers_free_themselves_and_views_free_nothing():
    """tests/fuzz/devbuf_unit.cpp (`make -C tests/fuzz devbuf_unit`: ctx.h against the stand-in runtime, under AddressSanitizer and UBSan, a program of its own) checks
    ensure / grow / release / scope exit of both buffer types, alias() and an outgrown alias, whole objects deleted with some of their buffers allocated, and
    Installed::borrow_from before and after the parent replaces a table -- each by the stand-in runtime's count of live allocations.  Done = exit status 0."""
    subprocess.check_call(["make", "-C", FUZZ, "-s", "devbuf_unit"])
    r = subprocess.run([os.path.join(FUZZ, "devbuf_unit")], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
