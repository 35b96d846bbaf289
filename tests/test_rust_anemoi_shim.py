"""The Rust side of the Anemoi layer, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain here): the
wrappers of uzkge-gpu-sys call the six new entry points with the arity the header declares, and rust/uzkge-glue/gpu_anemoi.rs calls
wrappers that exist, with the argument count they take, and nothing that can panic."""
import os
import re

from test_rust_shim import ROOT, RUST, _calls, _ffi, _strip_rust_comments

NEW = ("uzk_anemoi_permute_batch", "uzk_anemoi_hash_batch", "uzk_anemoi_stream_batch", "uzk_anemoi_permutations", "uzk_cp_reveal_prove0_batch",
       "uzk_cp_reveal_verify0_batch")


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def _header_arity():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "uzkge_gpu.h")).read(), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\b(uzk_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr)}


def test_the_new_entry_points_are_bound_and_wrapped_with_the_headers_arity():
    ffi, header = _ffi(), _header_arity()
    decl = {m.group(1): (0 if not m.group(2).strip() else m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    used = dict(_calls(_lib(), r"uzk_[a-z0-9_]+"))
    want = {"uzk_anemoi_permute_batch": 3, "uzk_anemoi_hash_batch": 5, "uzk_anemoi_stream_batch": 6, "uzk_anemoi_permutations": 2,
            "uzk_cp_reveal_prove0_batch": 7, "uzk_cp_reveal_verify0_batch": 5}
    for name in NEW:
        assert header.get(name) == want[name] == decl.get(name), (name, header.get(name), decl.get(name))
        assert used.get(name) == decl[name], (name, used.get(name), decl[name])
        assert re.search(rf"pub fn {name[4:]}\(", _lib()), name            # the safe wrapper carries the entry point's name
    for const in ("UZK_ANEMOI_MAX_BATCH", "UZK_ANEMOI_MAX_INPUT", "UZK_ANEMOI_MAX_OUTPUT", "UZK_ANEMOI_TRACE_ELEMS"):
        assert f"pub const {const}" in ffi, const
    assert "pub type AnemoiTraceBlock = [Limbs; 64];" in _lib()
    # the zk-friendly reveals take what the Keccak ones take
    sig = lambda name: re.search(rf"pub fn {name}\((.*?)\) -> (.*?) \{{", _lib()).groups()
    assert sig("cp_reveal_prove0_batch") == sig("cp_reveal_prove_batch") and sig("cp_reveal_verify0_batch") == sig("cp_reveal_verify_batch")


def test_the_anemoi_glue_calls_wrappers_that_exist():
    lib = _lib()
    glue = _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_anemoi.rs")).read())
    for fn in ("pub fn gpu_hash_batch(", "pub fn gpu_stream_cipher_with_trace(", "pub fn gpu_reveal_cards0<", "pub fn gpu_verify_reveals0("):
        assert fn in glue, fn
    wrappers = {}
    for m in re.finditer(r"pub fn ([a-z_0-9]+)\(", lib):
        wrappers[m.group(1)] = _calls(lib[m.start():], r"fn " + m.group(1))[0][1]
    called = _calls(glue, r"sys::[a-z_0-9]+")
    assert {n for n, _ in called} == {"sys::anemoi_hash_batch", "sys::anemoi_stream_batch", "sys::anemoi_permutations", "sys::cp_reveal_prove0_batch",
                                      "sys::cp_reveal_verify0_batch"}
    for name, n_args in called:
        assert wrappers[name.split("::")[1]] == n_args, (name, n_args)
    ffi = _ffi()
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    for t in re.findall(r"sys::([A-Z][a-z][A-Za-z]+)", glue):
        assert re.search(rf"pub type {t} ", lib), t
    # marshals to and from the reference's types, fills the five fields of the trace; a device error is None, never a panic
    assert "AnemoiStreamCipherTrace::<Fr, 2, N_ANEMOI_ROUNDS>::default()" in glue and "ChaumPedersenDLProof::from_uncompress" in glue
    for field in ("trace.input", "trace.before_permutation", "trace.intermediate_values_before_constant_additions", "trace.after_permutation", "trace.output"):
        assert field in glue, field
    assert "pair(b, 0)" in glue and "pair(b, 4 + 4 * r)" in glue and "pair(b, 60)" in glue      # the header's trace layout
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)", glue)
    assert "[point_to_wire(&masked.e1), point_to_wire(reveal), point_to_wire(pk)]" in glue
