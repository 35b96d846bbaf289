"""The Rust side of the reveal circuit, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain here): the
wrappers of uzkge-gpu-sys call the seven new entry points with the arity the generated bindings declare, rust/uzkge-glue/
gpu_reveal_snark.rs calls wrappers that exist with the argument count they take and nothing that can panic, ffi.rs equals the
regenerated bindings, and the patch with its new Cargo hook still applies."""
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_rust_shim import PATCHED, ROOT, RUST, _calls, _ffi, _strip_rust_comments

NEW = ("uzk_reveal_cs_info", "uzk_reveal_cs_matrices", "uzk_reveal_circuit_create", "uzk_reveal_circuit_release", "uzk_reveal_circuit_key",
       "uzk_reveal_witness_batch", "uzk_reveal_prove_snark_batch")


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def _glue():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_reveal_snark.rs")).read())


def test_the_bindings_are_the_regenerated_ones():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"]).returncode == 0


def test_the_new_entry_points_are_bound_and_wrapped():
    ffi = _ffi()
    decl = {m.group(1): (0 if not m.group(2).strip() else m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    used = dict(_calls(_lib(), r"uzk_[a-z0-9_]+"))
    for name in NEW:
        assert name in decl, name
        assert used.get(name) == decl[name], (name, used.get(name), decl[name])
    assert [decl[n] for n in NEW] == [5, 3, 2, 1, 2, 6, 8]
    for const in ("UZK_REVEAL_CS_VARS", "UZK_REVEAL_CS_INPUTS", "UZK_REVEAL_CS_MAX_BATCH"):
        assert f"pub const {const}" in ffi, const
    lib = _lib()
    assert "pub struct RevealCircuit {" in lib and "impl Drop for RevealCircuit {" in lib and "pub struct RevealWitness {" in lib
    drop = lib[lib.index("impl Drop for RevealCircuit {"):]
    assert "uzk_reveal_circuit_release(self.handle)" in drop[:drop.index("\n}\n")]
    assert "pub type RevealSnarkStatement = [Limbs; 6];" in lib


def test_the_glue_calls_wrappers_that_exist():
    lib, glue = _lib(), _glue()
    assert "pub fn gpu_reveal_cards_with_snark<" in glue and "pub fn gpu_reveal_circuit(" in glue
    body = lib[lib.index("impl RevealCircuit {"):lib.index("impl Drop for RevealCircuit {")]
    methods = {m.group(1): _calls(body[m.start():], r"fn " + m.group(1))[0][1] for m in re.finditer(r"pub fn ([a-z_0-9]+)\(", body)}
    assert methods["create"] == 1 and methods["prove_snark_batch"] == 5 and methods["witness_batch"] == 3        # &self counts
    assert dict(_calls(glue, r"sys::RevealCircuit::create")) == {"sys::RevealCircuit::create": 1}
    assert dict(_calls(glue, r"circuit\.prove_snark_batch")) == {"circuit.prove_snark_batch": 4}
    ffi = _ffi()
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    for t in set(re.findall(r"sys::(uzk_[a-z0-9_]+)\b", glue)):
        assert f"pub struct {t} " in ffi, t
    # every field of the descriptor the glue fills is a field of the generated struct, and none is left out
    desc = ffi[ffi.index("pub struct uzk_g16_key_desc {"):]
    fields = re.findall(r"pub ([a-z_0-9]+):", desc[:desc.index("}")])
    filled = glue[glue.index("sys::uzk_g16_key_desc {"):glue.index("sys::RevealCircuit::create(")]
    assert re.findall(r"^        ([a-z_0-9]+):", filled, flags=re.M) == fields
    assert filled.count("std::ptr::null()") == 3                                        # the matrices are the circuit's own
    # the blinds in the prover's order, the statement's order of the header, no panic
    assert glue.index("r.push((ScalarFr::rand(prng)") < glue.index("s.push((ScalarFr::rand(prng)")
    assert "point_from_wire(&st[4], &st[5]) != keypair.public" in glue and "point_from_wire(&st[2], &st[3])" in glue
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)", glue)


def test_the_patch_carries_the_cargo_hook():
    patch = open(os.path.join(RUST, "uzkge-gpu.patch")).read()
    assert '+uzkge-gpu-sys = { path = "../uzkge-gpu-sys", optional = true }' in patch
    assert '+gpu-reveal-snark = ["gpu", "uzkge-gpu-sys"]' in patch and '+gpu = ["uzkge/gpu"]' in patch


@pytest.mark.skipif(not os.path.isdir("/root/reference/uzkge"), reason="reference tree not present (GPU box)")
def test_the_patch_still_applies(tmp_path):
    if not shutil.which("patch"):
        pytest.skip("no patch(1)")
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "make_rust_patch.py"), "--check"]).returncode == 0
    for f in PATCHED:
        dst = tmp_path / f
        dst.parent.mkdir(parents=True, exist_ok=True)
        shutil.copy(os.path.join("/root/reference", f), dst)
    r = subprocess.run(["patch", "-p1", "-i", os.path.join(RUST, "uzkge-gpu.patch")], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    cargo = open(tmp_path / "shuffle/Cargo.toml").read()
    assert cargo.index("[dependencies]") < cargo.index("uzkge-gpu-sys = {") < cargo.index("[features]") < cargo.index("gpu-reveal-snark = [")
    # the glue names items of the reference: they exist where it looks for them
    src = open("/root/reference/shuffle/src/lib.rs").read() + open("/root/reference/shuffle/src/keygen.rs").read()
    for item in ("MaskedCard", "RevealCard", "pub struct Keypair", "pub secret", "pub public"):
        assert item in src, item
