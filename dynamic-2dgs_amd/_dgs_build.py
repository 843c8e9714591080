"""In-tree builds of the native libraries, keyed on a HASH of their inputs (sources, headers, compiler flags).

A library is rebuilt when the hash recorded next to it (`<lib>.srchash`) differs from the hash of the current inputs --
file times do not matter, so a checkout, a copy to the GPU box or a touched file can neither force nor hide a rebuild.
`source_hash()` is also what bench.py compares against the hash stored with the PMC traffic figures under profiles/.

Several processes may ask for the same library at once (N ranks of a torchrun launch whose binaries are stale or whose
`.srchash` files did not travel): builds are serialised by an exclusive `flock` on `<lib>.lock`, the compiler writes to a
temporary file in the same directory and the result is moved into place with `os.replace` (atomic on one file system), and
the hash is recorded only after that -- a process that `dlopen`s the path sees either the old complete file or the new
complete file, never a half-written one, and the ranks that waited for the lock find the hash current and reuse the binary.

`NativeLibrary` is the one description of a library the bindings share: where it lives, what it is built from, its prototypes,
and the life cycle from those (build, stale check, dlopen, prototypes, ABI check, error check).  No torch at import.
"""
import ctypes
import fcntl
import hashlib
import os
import subprocess


def source_hash(deps, flags):
    h = hashlib.sha256()
    h.update(("\0".join(flags)).encode())
    for d in deps:
        h.update(b"\0" + os.path.basename(d).encode() + b"\0")
        with open(d, "rb") as f:
            h.update(f.read())
    return h.hexdigest()[:16]


def recorded_hash(lib_path):
    try:
        with open(lib_path + ".srchash") as f:
            return f.read().strip()
    except OSError:
        return None


def _current(lib_path, want):
    return os.path.exists(lib_path) and recorded_hash(lib_path) == want


def build(lib_path, cmd, deps, flags, cwd, force=False, verbose=False):
    """Run `cmd` (which must name lib_path as its output) unless lib_path was built from exactly these inputs.
    Returns (lib_path, "compiled" | "reused").  Safe against concurrent callers (module docstring)."""
    want = source_hash(deps, flags)
    if not force and _current(lib_path, want):
        if verbose:
            print("[build] reused   %s (inputs %s)" % (os.path.basename(lib_path), want))
        return lib_path, "reused"
    assert lib_path in cmd, "the build command must name the library as its output"
    with open(lib_path + ".lock", "w") as lock:
        fcntl.flock(lock, fcntl.LOCK_EX)
        try:
            # somebody else may have built it while this process waited for the lock
            if not force and _current(lib_path, want):
                if verbose:
                    print("[build] reused   %s (inputs %s, built by another process)" % (os.path.basename(lib_path), want))
                return lib_path, "reused"
            tmp = "%s.tmp%d" % (lib_path, os.getpid())
            tmp_cmd = [tmp if c == lib_path else c for c in cmd]
            if verbose:
                print("[build] compiling %s (inputs %s): %s" % (os.path.basename(lib_path), want, " ".join(cmd)))
            try:
                subprocess.check_call(tmp_cmd, cwd=cwd)
                os.replace(tmp, lib_path)
            finally:
                if os.path.exists(tmp):
                    os.unlink(tmp)
            with open(lib_path + ".srchash.tmp%d" % os.getpid(), "w") as f:
                f.write(want + "\n")
            os.replace(lib_path + ".srchash.tmp%d" % os.getpid(), lib_path + ".srchash")
        finally:
            fcntl.flock(lock, fcntl.LOCK_UN)
    return lib_path, "compiled"


def stream(device):
    """The current HIP stream of `device` as the void* the C entry points take."""
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


class NativeLibrary:
    """default_path: where build() puts the library; `env` names an environment variable that may point load() at a caller's own
    build instead.  inputs: the ORDERED list of files the hash covers (the order is part of the hash); `main` is the one handed to
    the compiler.  signatures: {name: (restype, argtypes)} of every function of the public header.  abi: (function, wanted
    version); last_error: the function check() reads the message from."""

    def __init__(self, default_path, main, inputs, flags, signatures, abi, last_error, env=None, compiler=("hipcc",),
                 missing="%s not found; build it with __graft_entry__.build()", failed="%s failed (%d): %s"):
        self.default_path = default_path
        self.path = os.environ.get(env, default_path) if env else default_path
        self.main, self.inputs, self.flags, self.signatures = main, list(inputs), list(flags), signatures
        (self.abi_fn, self.abi_version), self.last_error = abi, last_error
        self.compiler, self.missing, self.failed = list(compiler), missing, failed
        self._lib = None

    def deps(self):
        return list(self.inputs)

    def source_hash(self):
        """Hash of the sources + flags the library is built from (recorded next to the .so and with the PMC profiles)."""
        return source_hash(self.inputs, self.flags)

    def build(self, force=False, verbose=False):
        """Compile the library in-tree at its default path.  Rebuilds whenever the hash of sources + flags differs from the one
        recorded with the existing binary."""
        cmd = self.compiler + self.flags + [self.main, "-o", self.default_path]
        return build(self.default_path, cmd, self.inputs, self.flags, os.path.dirname(self.main), force=force, verbose=verbose)[0]

    def _rebuild_if_stale(self):
        """A binary built from other sources than the ones in the tree must never be what the tests or the bench measure: if the
        hash recorded next to it differs from the hash of the current sources + flags, rebuild; if that is impossible, fail.
        Only the default path is ours to judge: any other path is a caller's own build (an A/B build through `env`, or a twin
        with its own flags) and the caller's responsibility."""
        if os.path.abspath(self.path) != os.path.abspath(self.default_path):
            return
        have, want = recorded_hash(self.path), self.source_hash()
        if have == want:
            return
        try:
            self.build()
        except Exception as ex:
            raise RuntimeError("%s was built from other sources (recorded inputs %s, tree %s) and cannot be rebuilt here: %r"
                               % (self.path, have, want, ex))

    def load(self):
        """dlopen the library and declare the prototypes of its public header."""
        if self._lib is None:
            if not os.path.exists(self.path):
                raise RuntimeError(self.missing % self.path)
            self._rebuild_if_stale()
            lib = ctypes.CDLL(self.path)
            for name, (restype, argtypes) in self.signatures.items():
                f = getattr(lib, name)
                f.restype, f.argtypes = restype, argtypes
            have = getattr(lib, self.abi_fn)()
            if have != self.abi_version:
                raise RuntimeError("%s ABI version mismatch (want %d, library says %d): rebuild it"
                                   % (os.path.basename(self.default_path), self.abi_version, have))
            self._lib = lib
        return self._lib

    def check(self, rc, what):
        if rc < 0:
            raise RuntimeError(self.failed % (what, rc, getattr(self.load(), self.last_error)().decode("utf-8", "replace")))
