"""The Rust side of the Baby Jubjub layer, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain here):
the wrappers of uzkge-gpu-sys call the six new entry points with the arity the generated bindings declare, and
rust/uzkge-glue/gpu_reveal.rs calls wrappers that exist, with the argument count they take, and nothing that can panic."""
import os
import re

from test_rust_shim import RUST, _calls, _ffi, _strip_rust_comments

NEW = ("uzk_ed_check_points", "uzk_ed_mul_batch", "uzk_ed_sum_batch", "uzk_ed_unmask_batch", "uzk_cp_reveal_prove_batch", "uzk_cp_reveal_verify_batch")


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def test_the_new_entry_points_are_bound_and_wrapped():
    ffi = _ffi()
    decl = {m.group(1): (0 if not m.group(2).strip() else m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    used = dict(_calls(_lib(), r"uzk_[a-z0-9_]+"))
    for name in NEW:
        assert name in decl, name
        assert used.get(name) == decl[name], (name, used.get(name), decl[name])
        assert re.search(rf"pub fn {name[4:]}\(", _lib()), name            # the safe wrapper carries the entry point's name
    for const in ("UZK_CP_PROOF_BYTES", "UZK_CP_MAX_BATCH", "UZK_ED_MAX_BATCH", "UZK_ED_MAX_ROWS"):
        assert f"pub const {const}" in ffi, const
    assert "pub type EdPoint = [Limbs; 2];" in _lib() and "pub type RevealStatement = [EdPoint; 3];" in _lib()


def test_the_reveal_glue_calls_wrappers_that_exist():
    lib = _lib()
    glue = _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_reveal.rs")).read())
    assert "pub fn gpu_reveal_cards<" in glue and "pub fn gpu_verify_reveals_cp(" in glue
    wrappers = {}
    for m in re.finditer(r"pub fn ([a-z_0-9]+)\(", lib):
        wrappers[m.group(1)] = _calls(lib[m.start():], r"fn " + m.group(1))[0][1]
    called = _calls(glue, r"sys::[a-z_0-9]+")
    assert {n for n, _ in called} == {"sys::cp_reveal_prove_batch", "sys::cp_reveal_verify_batch"}
    for name, n_args in called:
        assert wrappers[name.split("::")[1]] == n_args, (name, n_args)
    ffi = _ffi()
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    for t in re.findall(r"sys::([A-Z][a-z][A-Za-z]+)", glue):
        assert re.search(rf"pub type {t} ", lib), t
    # marshals to and from the reference's types; a device error is None, never a panic (the workspace builds with panic = "abort")
    assert "EdwardsProjective" in glue and "ChaumPedersenDLProof::from_uncompress" in glue and "to_uncompress()" in glue
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)", glue)
    # the statement order of the header: e1, reveal, pk
    assert "[point_to_wire(&masked.e1), point_to_wire(reveal), point_to_wire(pk)]" in glue
