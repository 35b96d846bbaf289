"""The Rust side of the point codec, checked textually like the rest of rust/ (tests/test_rust_shim.py; no Rust toolchain here): ffi.rs
equals the regenerated bindings and declares the eleven new entry points with the header's arity (and no parameter named by a Rust
keyword), the wrappers of uzkge-gpu-sys call what they say they call with that arity, and rust/uzkge-glue/gpu_codec.rs calls
wrappers that exist with the argument count they take and nothing that can panic."""
import os
import re
import subprocess
import sys

from test_rust_shim import ROOT, RUST, _calls, _ffi, _strip_rust_comments

NEW = {"uzk_g1_decompress_batch": 4, "uzk_g2_decompress_batch": 5, "uzk_ed_decompress_batch": 5, "uzk_g1_compress_batch": 4, "uzk_g2_compress_batch": 4,
       "uzk_ed_compress_batch": 4, "uzk_srs_register_compressed": 3, "uzk_g2_register_compressed": 4, "uzk_g16_pk_layout": 3,
       "uzk_g16_vk_create_compressed": 4, "uzk_reveal_circuit_create_compressed": 4}
WRAPPED = {"g1_decompress": "uzk_g1_decompress_batch", "g2_decompress": "uzk_g2_decompress_batch", "ed_decompress": "uzk_ed_decompress_batch",
           "g1_compress": "uzk_g1_compress_batch", "g2_compress": "uzk_g2_compress_batch", "ed_compress": "uzk_ed_compress_batch",
           "g16_pk_layout": "uzk_g16_pk_layout"}


def _lib():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-gpu-sys", "src", "lib.rs")).read())


def _glue():
    return _strip_rust_comments(open(os.path.join(RUST, "uzkge-glue", "gpu_codec.rs")).read())


def _header_arity():
    hdr = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "uzkge_gpu.h")).read(), flags=re.S)
    return {m.group(1): m.group(2).count(",") + 1 for m in re.finditer(r"\bint (uzk_[a-z0-9_]+)\s*\(([^;{}]*?)\)\s*;", hdr)}


def test_the_bindings_are_the_regenerated_ones():
    assert subprocess.run([sys.executable, os.path.join(ROOT, "tools", "gen_rust_bindings.py"), "--check"]).returncode == 0


def test_the_new_entry_points_are_bound_with_the_headers_arity():
    ffi, hdr = _ffi(), _header_arity()
    decl = {m.group(1): (m.group(2), m.group(2).count(",") + 1) for m in re.finditer(r"pub fn (uzk_[a-z0-9_]+)\((.*?)\)", ffi)}
    for name, arity in NEW.items():
        assert hdr.get(name) == arity, (name, hdr.get(name))
        assert name in decl and decl[name][1] == arity, name
        params = re.findall(r"(\w+):", decl[name][0])
        assert not set(params) & {"in", "type", "ref", "match", "move", "fn", "mod", "use", "loop", "box"}, (name, params)
    assert "pub const UZK_CODEC_MAX_BATCH: c_int = 1048576;" in ffi and "pub const UZK_G16_PK_SECTIONS: c_int = 12;" in ffi
    assert [f"pub const UZK_PK_{n}: c_int = {k};" in ffi for k, n in enumerate(
        ("ALPHA_G1", "BETA_G2", "GAMMA_G2", "DELTA_G2", "GAMMA_ABC_G1", "BETA_G1", "DELTA_G1", "A_QUERY", "B_G1_QUERY", "B_G2_QUERY", "H_QUERY", "L_QUERY"))] == [True] * 12
    st = ffi[ffi.index("pub struct uzk_g16_pk_sections {"):]
    assert re.findall(r"pub ([a-z_]+): ([^,]+),", st[:st.index("}")]) == [("offset", "[u64; UZK_G16_PK_SECTIONS as usize]"), ("count", "[u64; UZK_G16_PK_SECTIONS as usize]"),
                                                                          ("infinities", "[u64; UZK_G16_PK_SECTIONS as usize]"), ("bytes", "u64")]
    import ctypes
    from uzkge_amd._native import G16PkSections
    assert ctypes.sizeof(G16PkSections) == 8 * (3 * 12 + 1)


def test_the_wrappers_call_what_they_say_they_call():
    lib = _lib()
    mod = lib[lib.index("pub mod codec {"):]
    for wrapper, entry in WRAPPED.items():
        body = mod[mod.index(f"pub fn {wrapper}("):]
        body = body[:body.index("\n    }\n")]
        calls = dict(_calls(body, r"uzk_[a-z0-9_]+"))
        calls.pop("uzk_g1_affine", None), calls.pop("uzk_g2_affine", None), calls.pop("uzk_g16_pk_sections", None)
        assert calls == {entry: NEW[entry]}, (wrapper, calls)
    for ty, entry, release in (("Groth16Vk", "uzk_g16_vk_create_compressed", "uzk_g16_vk_release"),
                               ("RevealCircuit", "uzk_reveal_circuit_create_compressed", "uzk_reveal_circuit_release")):
        imp = lib[lib.index(f"impl {ty} {{"):]
        body = imp[imp.index("pub fn from_compressed("):]
        body = body[:body.index("\n    }\n")]
        calls = dict(_calls(body, r"uzk_[a-z0-9_]+"))
        assert calls[entry] == NEW[entry] and release in calls, (ty, calls)            # a handle that cannot be described is released
        assert _calls(body, r"fn from_compressed")[0][1] == 2


def test_the_glue_calls_wrappers_that_exist():
    lib, glue, ffi = _lib(), _glue(), _ffi()
    for fn in ("pub fn gpu_load_reveal_key(", "pub fn gpu_points_from_hex("):
        assert fn in glue, fn
    assert _calls(glue, r"fn gpu_load_reveal_key")[0][1] == 2 and _calls(glue, r"fn gpu_points_from_hex")[0][1] == 1
    mod = lib[lib.index("pub mod codec {"):]
    for name, n_args in _calls(glue, r"sys::codec::[a-z_0-9]+"):
        short = name.split("::")[2]
        assert _calls(mod[mod.index(f"pub fn {short}("):], r"fn " + short)[0][1] == n_args, (name, n_args)
    assert dict(_calls(glue, r"sys::RevealCircuit::from_compressed")) == {"sys::RevealCircuit::from_compressed": 2}
    assert dict(_calls(glue, r"sys::codec::ed_decompress")) == {"sys::codec::ed_decompress": 2} and "ed_decompress(&enc, true)" in glue
    for c in re.findall(r"sys::(UZK_[A-Z0-9_]+)", glue):
        assert f"pub const {c}" in ffi, c
    assert not re.search(r"\bassert(_eq)?!|\.expect\(|panic!|\.unwrap\(\)|\[\s*\.\.", glue)
