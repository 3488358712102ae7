"""The generated FFI crate (rust/bzk-sys/src/lib.rs) as Rust a compiler would take: every struct field is `pub <identifier>: <type>,` - there is
no rustc in the test image, and tests/test_rust_shim_cpu.py only compares the file with the generator's output - and an array inside a C struct
is an array inside the Rust one, with the C layout."""
import ctypes as C
import os
import re

from bazuka_amd import lib as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYS_RS = os.path.join(ROOT, "rust", "bzk-sys", "src", "lib.rs")
TYPE = r"(\*(const|mut) )*\w+"


def structs():
    src = open(SYS_RS).read()
    return {m.group(1): [ln.strip() for ln in m.group(2).strip().splitlines()] for m in re.finditer(r"pub struct (\w+) \{\n(.*?)\n\}", src, re.S)}


def test_every_struct_field_is_an_identifier_with_a_type():
    found = structs()
    assert len(found) >= 3 and "bzk_contract_desc" in found
    for name, fields in found.items():
        assert fields, name
        for f in fields:
            assert re.fullmatch(r"pub (r#)?[A-Za-z_]\w*: (%s|\[%s; \d+\])," % (TYPE, TYPE), f), (name, f)


def test_contract_desc_layout():
    fields = structs()["bzk_contract_desc"]
    assert fields[0] == "pub contract_id: [u8; 32],"
    assert [f.split(":")[0] for f in fields] == ["pub " + n for n, _ in L._ContractDescStruct._fields_]
    # the C layout the Rust declaration has to reproduce: 32 bytes, then pointer / count pairs
    assert L._ContractDescStruct.contract_id.size == 32 and L._ContractDescStruct.deposit_fns.offset == 32
    assert C.sizeof(L._ContractDescStruct) == 32 + 3 * 16 and C.sizeof(L._ContractFn) == 24
