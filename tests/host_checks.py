"""What the CPU tests of the C ABI's host-side argument checks share (tests/test_*_cpu.py): one bad argument through both views of a header.
A plain module: not collected, no tests of its own.  The tables of good and bad arguments stay with the feature they belong to."""
import pytest


def assert_host_check_fails(raw, checked, name, args, word=""):
    """``name(*args)`` is refused before any HIP call: the raw view returns EMAP_E_INVALID and ``emap_last_error()`` starts with the entry
    point's name (and holds ``word``); the checked view raises with that text."""
    entry = name[len("emap_"):]
    assert getattr(raw, name)(*args) == -1
    msg = raw.emap_last_error().decode()
    assert msg.startswith(entry + ":") and word in msg, msg
    with pytest.raises(RuntimeError, match=rf"{entry} failed \(rc=-1\): {entry}:"):
        getattr(checked, entry)(*args)
