"""CPU: tools/kernel_isa_diff.py on hand-written assembly of a few instructions.  The same body under another name,
in another file and with other label ordinals is a match; one changed register is reported and fails the run; so does a
kernel that only one side has."""
import importlib.util
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
spec = importlib.util.spec_from_file_location("kernel_isa_diff", os.path.join(ROOT, "tools", "kernel_isa_diff.py"))
isa = importlib.util.module_from_spec(spec)
spec.loader.exec_module(isa)

BODY = """\
\t.globl\t{name} ; -- Begin function {name}
\t.p2align\t8
\t.type\t{name},@function
{name}: ; @{name}
; %bb.0:
\ts_load_dwordx2 s[0:1], s[0:1], 0x0
\tv_lshlrev_b32_e32 v0, 3, v0
\tv_cmp_gt_u32_e32 vcc, 64, v0 ; a comment
\ts_and_saveexec_b64 s[2:3], vcc

\ts_cbranch_execz .LBB{fn}_{l1}
; %bb.1:
\tv_add_f64 {reg}, v[2:3], v[2:3]
\ts_getpc_b64 s[4:5]
\ts_add_u32 s4, s4, {name}.helper@rel32@lo+4
.LBB{fn}_{l0}: ; %loop
\tv_add_u32_e32 v0, 1, v0
\ts_cbranch_scc1 .LBB{fn}_{l0}
.LBB{fn}_{l1}:
\ts_endpgm
\t.section\t.rodata,"a",@progbits
.Lfunc_end{fn}:
\t.size\t{name}, .Lfunc_end{fn}-{name}
"""
META = """\
  - .agpr_count:     0
    .args:
      - .offset:         0
        .size:           8
        .name:           not_a_kernel
    .group_segment_fixed_size: {lds}
    .name:           {name}
    .private_segment_fixed_size: 0
    .sgpr_count:     12
    .symbol:         {name}.kd
    .vgpr_count:     {vgprs}
"""


def asm(*kernels):
    """One .s file: kernels = (name, function ordinal, label ordinals, the register of one instruction, vgprs)"""
    text = "\t.text\n" + "".join(BODY.format(name=n, fn=fn, l0=l[0], l1=l[1], reg=reg) for n, fn, l, reg, _ in kernels)
    meta = "".join(META.format(name=n, lds=0, vgprs=v) for n, _, _, _, v in kernels)
    return text + "\t.amdgpu_metadata\n---\namdhsa.kernels:\n" + meta + "amdhsa.target:   amdgcn-amd-amdhsa--gfx950\n...\n"


def run(tmp_path, capsys, old_files, new_files, *extra):
    for side, files in (("old", old_files), ("new", new_files)):
        os.makedirs(tmp_path / side)
        for name, text in files.items():
            (tmp_path / side / name).write_text(text)
    status = isa.main([str(tmp_path / "old"), str(tmp_path / "new"), *extra])
    return status, capsys.readouterr().out


def test_same_body_other_name_file_and_labels(tmp_path, capsys):
    old = {"one.s": asm(("_Z3fooILb1EEvv", 0, (3, 1), "v[4:5]", 6), ("_Z3barv", 1, (2, 0), "v[6:7]", 8))}
    new = {"a.s": asm(("_Z3barv", 0, (1, 5), "v[6:7]", 8)), "b.s": asm(("_Z7foo_newvv", 4, (0, 2), "v[4:5]", 6))}
    status, out = run(tmp_path, capsys, old, new)
    assert status == 0
    assert "a.s: _Z3barv: identical to one.s: _Z3barv" in out
    assert "b.s: _Z7foo_newvv: identical to one.s: _Z3fooILb1EEvv" in out
    assert "no match" not in out and "not_a_kernel" not in out
    assert "2 kernels old, 2 new, 0 without a partner" in out


def test_one_changed_register(tmp_path, capsys):
    old = {"one.s": asm(("_Z3foov", 0, (0, 1), "v[4:5]", 6))}
    new = {"one.s": asm(("_Z3foov", 0, (0, 1), "v[8:9]", 10))}
    status, out = run(tmp_path, capsys, old, new)
    assert status != 0
    assert "one.s: _Z3foov: no match\n" in out
    assert ".vgpr_count 10" in out and ".vgpr_count 6" in out          # both sides' resources
    assert "-v_add_f64 v[4:5], v[2:3], v[2:3]" in out and "+v_add_f64 v[8:9], v[2:3], v[2:3]" in out
    assert "no match (on the old side only)" in out
    assert "2 without a partner" in out


def test_kernel_on_one_side_only(tmp_path, capsys):
    both = ("_Z3foov", 0, (0, 1), "v[4:5]", 6)
    extra = ("_Z5extrav", 1, (0, 1), "v[10:11]", 12)
    status, out = run(tmp_path, capsys, {"one.s": asm(both)}, {"one.s": asm(both, extra)})
    assert status != 0
    assert "one.s: _Z3foov: identical to one.s: _Z3foov" in out and "one.s: _Z5extrav: no match\n" in out
    status, out = run(tmp_path / "swapped", capsys, {"one.s": asm(both, extra)}, {"one.s": asm(both)})
    assert status != 0 and "one.s: _Z5extrav: no match (on the old side only)" in out
    # --only leaves the kernel out of the comparison on both sides
    status, out = run(tmp_path / "only", capsys, {"one.s": asm(both, extra)}, {"one.s": asm(both)}, "--only", "*foo*")
    assert status == 0 and "extra" not in out
