"""The Rust side of the matchmaking circuit, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain
here): the wrappers of uzkge-gpu-sys call the three new entry points with the arity the generated bindings declare, and
rust/uzkge-glue/gpu_matchmaking.rs calls wrappers that exist, with the argument count they take, and nothing that can panic."""
import os
import re

from test_rust_shim import RUST, _calls, _ffi, _strip_rust_comments

NEW = {"uzk_match_cs_info": 6, "uzk_match_circuit_create": 3, "uzk_match_witness_batch": 10}


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def _glue():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_matchmaking.rs")).read())


def test_the_new_entry_points_are_bound_and_wrapped():
    ffi, lib = _ffi(), _lib()
    decl = {m.group(1): (0 if not m.group(2).strip() else m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    used = {}
    for name, n_args in _calls(lib, r"uzk_match_[a-z0-9_]+"):
        used.setdefault(name, set()).add(n_args)
    for name, arity in NEW.items():
        assert decl.get(name) == arity, (name, decl.get(name))
        assert used.get(name) == {arity}, (name, used.get(name))
    for const, value in (("UZK_MATCH_CS_MIN_PLAYERS", 3), ("UZK_MATCH_CS_MAX_PLAYERS", 64), ("UZK_MATCH_CS_MAX_BATCH", 1024), ("UZK_MATCH_CS_KEY_COMMITMENTS", 19)):
        assert "pub const %s: c_int = %d;" % (const, value) in ffi
    assert "pub struct uzk_match_circuit_desc {" in ffi and "pub players: u32," in ffi
    # the test hooks of include/uzkge_gpu_test.h are not part of the drop-in ABI
    assert "uzk_test_match" not in ffi and "uzk_test_match" not in lib
    # the circuit is a handle with a Drop that releases it, the witness frees its device memory
    assert "pub struct MatchCircuit {" in lib and re.search(r"impl Drop for MatchCircuit \{\s*fn drop\(&mut self\) \{\s*unsafe \{ uzk_circuit_release\(self\.handle\) \};", lib)
    assert "pub struct MatchWitness {" in lib and re.search(r"impl Drop for MatchWitness \{\s*fn drop\(&mut self\) \{\s*unsafe \{ uzk_dev_free\(self\.d_witness\) \};", lib)
    for fn in ("pub fn match_cs_info(players: u32)", "pub fn create(desc: &uzk_match_circuit_desc)", "pub fn witness_batch(&self, inputs: &[Limbs], seeds: &[Limbs], randoms: &[Limbs])"):
        assert fn in lib, fn
    # the sizes the wrapper allocates are the header's: 5 n elements per match, 2 players + 2 online inputs
    assert "uzk_dev_alloc(32 * 5 * n * batch, &mut w.d_witness)" in lib and "batch * (2 * players + 2)" in lib


def test_the_matchmaking_glue_calls_wrappers_that_exist():
    lib, glue, ffi = _lib(), _glue(), _ffi()
    assert "pub fn gpu_match_witness(" in glue
    start = lib.index("impl MatchCircuit {")
    wrappers = {}
    for m in re.finditer(r"pub fn ([a-z_0-9]+)\(", lib[start:lib.index("impl Drop for MatchCircuit")]):
        wrappers[m.group(1)] = _calls(lib[start + m.start():], r"fn " + m.group(1))[0][1]
    assert _calls(glue, r"circuit\.witness_batch") == [("circuit.witness_batch", 3)] and wrappers["witness_batch"] == 4      # &self and three arguments
    assert _calls(glue, r"circuit\.players") == [("circuit.players", 0)] and wrappers["players"] == 1
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    for t in re.findall(r"sys::([A-Z][a-z][A-Za-z]+)", glue):
        assert re.search(rf"pub (type|struct) {t} ", lib), t
    # a device error is None, never a panic (the workspace builds with panic = "abort"); elements cross as Montgomery limbs
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)", glue)
    assert ".ok()?" in glue and "Fr::new_unchecked(BigInt(*w))" in glue and "(v.0).0" in glue
    assert "m.inputs.len() != players" in glue
