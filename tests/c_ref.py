"""The loader of the C restatements the tests compare against -- TEST INFRASTRUCTURE: tests/<name>.c compiled on the fly with
every operation rounded on its own (no contraction), once per process."""
import ctypes
import functools
import os
import subprocess
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))


@functools.lru_cache(maxsize=None)
def load(name):
    """The CDLL of tests/<name>.c."""
    out = os.path.join(tempfile.mkdtemp(prefix=name + "_"), name + ".so")
    subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, name + ".c"), "-o", out, "-lm"],
                   check=True)
    return ctypes.CDLL(out)
