"""The Rust side of the mask and the remask, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain
here): the wrappers of uzkge-gpu-sys call the six new entry points with the arity the generated bindings declare, and
rust/uzkge-glue/gpu_shuffle.rs calls wrappers that exist, with the argument count they take, and nothing that can panic."""
import os
import re

from test_rust_shim import RUST, _calls, _ffi, _strip_rust_comments

NEW = ("uzk_remark_key_create", "uzk_remark_key_release", "uzk_remark_key_tables", "uzk_remark_batch", "uzk_cp_mask_prove_batch", "uzk_cp_mask_verify_batch")


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def _glue():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_shuffle.rs")).read())


def test_the_new_entry_points_are_bound_and_wrapped():
    ffi, lib = _ffi(), _lib()
    decl = {m.group(1): (0 if not m.group(2).strip() else m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    want = {"uzk_remark_key_create": 2, "uzk_remark_key_release": 1, "uzk_remark_key_tables": 3, "uzk_remark_batch": 9, "uzk_cp_mask_prove_batch": 8,
            "uzk_cp_mask_verify_batch": 8}
    used = dict(_calls(lib, r"uzk_[a-z0-9_]+"))
    for name in NEW:
        assert decl.get(name) == want[name], (name, decl.get(name))
        assert used.get(name) == decl[name], (name, used.get(name), decl[name])
    assert "pub const UZK_REMARK_ITERATIONS: c_int = 84;" in ffi
    # the key is a handle with a Drop that releases it; the two mask calls carry the entry points' names
    assert "pub struct RemarkKey {" in lib and re.search(r"impl Drop for RemarkKey \{\s*fn drop\(&mut self\) \{\s*unsafe \{ uzk_remark_key_release\(self\.handle\) \};", lib)
    for fn in ("pub fn cp_mask_prove_batch(", "pub fn cp_mask_verify_batch(", "pub fn remark_batch(&self,", "pub fn tables(&self)", "pub fn new(pk: &EdPoint)"):
        assert fn in lib, fn
    # an optional pointer is null, never a dangling one
    assert "perm.map_or(std::ptr::null(), |p| p.as_ptr())" in lib and "map_or(std::ptr::null_mut()," in lib


def test_the_shuffle_glue_calls_wrappers_that_exist():
    lib, glue, ffi = _lib(), _glue(), _ffi()
    for fn in ("pub fn gpu_mask_cards<", "pub fn gpu_verify_masks(", "pub fn gpu_remark_deck("):
        assert fn in glue, fn
    wrappers = {}
    for m in re.finditer(r"pub fn ([a-z_0-9]+)\(", lib):
        wrappers[m.group(1)] = _calls(lib[m.start():], r"fn " + m.group(1))[0][1]
    called = _calls(glue, r"sys::[a-z_0-9]+")
    assert {n for n, _ in called} == {"sys::cp_mask_prove_batch", "sys::cp_mask_verify_batch"}
    for name, n_args in called:
        assert wrappers[name.split("::")[1]] == n_args, (name, n_args)
    method = _calls(glue, r"key\.remark_batch")
    assert method == [("key.remark_batch", 5)] and wrappers["remark_batch"] == 6          # &self and five arguments
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    for t in re.findall(r"sys::([A-Z][a-z][A-Za-z]+)", glue):
        assert re.search(rf"pub (type|struct) {t} ", lib), t
    # marshals to and from the reference's types; a device error is None, never a panic (the workspace builds with panic = "abort")
    for word in ("EdwardsProjective", "ChaumPedersenDLProof::from_uncompress", "to_uncompress()", "RemarkTrace {", "permutation.get_matrix()", "MaskedCard {"):
        assert word in glue, word
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)", glue)
    # the digit byte of the header, the reference's field bits (bits[2] false is minus one) and the trace's order as it comes
    assert "(bits[0] as u8) | ((bits[1] as u8) << 1) | ((bits[2] as u8) << 2)" in glue
    assert "if b[2] { one } else { -one }" in glue
    assert "[field(&t[0]), field(&t[1]), field(&t[2]), field(&t[3])]" in glue
    assert "n_round: iters" in glue and "Some(&perm), true" in glue
