"""Static guard on the shipped device code (VERDICT / ADVICE round 2): kernels built WITH packed-f32 VALU instructions
(v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32 / v_pk_mov_b32) were not bitwise repeatable at two waves per SIMD
(DESIGN.md section 9).  The Makefile disables the target feature; this test disassembles every gfx950 code object inside
libphnn_mpc.so and asserts that none of those opcodes is present -- so a toolchain bump, a dropped flag or a new
translation unit cannot re-introduce them silently.  It also pins the matrix instructions the design rests on, and what
the bit-exact model of k_lbfgs (tests/lbfgs_kernel_model.py) rests on: no contracted multiply-add in any k_lbfgs<E4>
instantiation, the only FMAs being those inside its three correctly rounded float32 divisions.  The same for k_adam and
its bit-exact model (tests/adam_model.py): two divisions, a correctly rounded square root, one fused lerp, nothing else fused.
"""
import os
import re
import struct
import subprocess
import tempfile

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "phnn_mpc_amd", "csrc", "libphnn_mpc.so")
LLVM = "/opt/rocm/lib/llvm/bin"
MAGIC = b"__CLANG_OFFLOAD_BUNDLE__"


def _code_objects(path):
    """gfx950 ELF images inside the library's .hip_fatbin section (one clang offload bundle per translation unit)."""
    blob = open(path, "rb").read()
    out, pos = [], blob.find(MAGIC)
    while pos >= 0:
        n = struct.unpack_from("<Q", blob, pos + len(MAGIC))[0]
        p = pos + len(MAGIC) + 8
        for _ in range(n):
            off, size, tlen = struct.unpack_from("<QQQ", blob, p)
            triple = blob[p + 24:p + 24 + tlen].decode()
            p += 24 + tlen
            if "gfx950" in triple and size > 0:
                out.append(blob[pos + off:pos + off + size])
        pos = blob.find(MAGIC, pos + len(MAGIC))
    return out


def _linked_units():
    """The translation units the Makefile links into libphnn_mpc.so (the .o prerequisites of its rule)."""
    mk = open(os.path.join(ROOT, "phnn_mpc_amd", "csrc", "Makefile")).read()
    rule = re.search(r"^libphnn_mpc\.so:(.*)$", mk, re.M)
    assert rule, "no libphnn_mpc.so rule in the Makefile"
    return [w for w in rule.group(1).split() if w.endswith(".o")]


@pytest.fixture(scope="module")
def disassembly():
    """llvm-objdump -d text of every gfx950 code object, one per linked translation unit."""
    if not os.path.exists(os.path.join(LLVM, "llvm-objdump")):
        pytest.skip("llvm-objdump not available")
    objs = _code_objects(LIB)
    units = _linked_units()
    assert len(objs) == len(units), f"expected one gfx950 code object per linked unit {units}, found {len(objs)}"
    out = []
    with tempfile.TemporaryDirectory() as tmp:
        for k, img in enumerate(objs):
            f = os.path.join(tmp, f"co{k}.elf")
            open(f, "wb").write(img)
            out.append(subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--mcpu=gfx950", f], capture_output=True,
                                      text=True, check=True).stdout)
    return out


@pytest.fixture(scope="module")
def opcodes(disassembly):
    counts = {}
    for txt in disassembly:
        for m in re.finditer(r"^\s+([sv]_[a-z0-9_]+|ds_[a-z0-9_]+|global_[a-z0-9_]+|scratch_[a-z0-9_]+|buffer_[a-z0-9_]+)\b", txt, re.M):
            counts[m.group(1)] = counts.get(m.group(1), 0) + 1
    return counts


def _functions(txt):
    """{symbol: [opcode, ...] in address order} of one disassembled code object; opcodes without their encoding
    suffix (_e32, _e64, _dpp, _sdwa)."""
    funcs, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+([sv]_[a-z0-9_]+)\b", line)
        if m and cur is not None:
            cur.append(re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)))
    return funcs


def _function_lines(txt):
    """{symbol: [(opcode, operands), ...] in address order}; opcodes without their encoding suffix."""
    funcs, cur = {}, None
    for line in txt.splitlines():
        m = re.match(r"^[0-9a-f]+ <([^>]+)>:", line)
        if m:
            cur = funcs.setdefault(m.group(1), [])
            continue
        m = re.match(r"^\s+([sv]_[a-z0-9_]+)\s*(.*?)\s*(//.*)?$", line)
        if m and cur is not None:
            cur.append((re.sub(r"_(e32|e64|dpp|sdwa)$", "", m.group(1)), m.group(2)))
    return funcs


def test_no_packed_f32_valu_in_device_code(opcodes):
    packed = {op: n for op, n in opcodes.items() if re.match(r"v_pk_(fma|mul|add)_f32|v_pk_mov_b32", op)}
    assert not packed, f"packed-f32 VALU instructions in the shipped device code (Makefile: NOPK flag lost?): {packed}"


def test_matrix_instructions_the_design_rests_on_are_present(opcodes):
    for op in ("v_mfma_f32_16x16x32_f16", "v_mfma_f32_16x16x32_bf16", "v_mfma_f32_16x16x4_f32", "v_mfma_f32_4x4x1_16b_f32",
               "ds_read_b64_tr_b16"):
        assert opcodes.get(op, 0) > 0, f"{op} missing from the device code"


def test_k_lbfgs_has_no_contracted_arithmetic(disassembly):
    """Every k_lbfgs<E4> (E4 = 1 .. 4): each v_fma_f32 / v_fmac_f32 and v_rcp_f32 lies inside a v_div_scale_f32 ...
    v_div_fixup_f32 window (a correctly rounded division), there are exactly three such windows (1/ys, ys/(y.y),
    1/sum|g|), and no v_mad_f32, v_mac_f32, v_fmamk_f32 or v_fmaak_f32 at all.  A dropped -ffp-contract=off or a
    fast-math flag breaks the bitwise model of tests/lbfgs_kernel_model.py; this catches it without a GPU."""
    kernels = {}
    for txt in disassembly:
        for name, ops in _functions(txt).items():
            m = re.fullmatch(r"_ZN12_GLOBAL__N_17k_lbfgsILi([1-4])EEEv11LbfgsParams", name)
            if m:
                kernels[int(m.group(1))] = ops
    assert sorted(kernels) == [1, 2, 3, 4], f"k_lbfgs instantiations found: {sorted(kernels)}"
    for e4, ops in sorted(kernels.items()):
        banned = sorted({op for op in ops if op in ("v_mad_f32", "v_mac_f32", "v_fmamk_f32", "v_fmaak_f32")})
        assert not banned, f"k_lbfgs<{e4}>: contracted multiply-add {banned}"
        windows, inside, fmas = 0, False, 0
        for op in ops:
            if op == "v_div_scale_f32":
                inside = True
            elif op == "v_div_fixup_f32":
                assert inside, f"k_lbfgs<{e4}>: v_div_fixup_f32 without v_div_scale_f32"
                windows, inside = windows + 1, False
            elif op in ("v_fma_f32", "v_fmac_f32", "v_rcp_f32"):
                assert inside, f"k_lbfgs<{e4}>: {op} outside a division"
                fmas += op != "v_rcp_f32"
        assert windows == 3, f"k_lbfgs<{e4}>: {windows} division windows, expected 3 (1/ys, ys/(y.y), 1/sum|g|)"
        assert fmas > 0, f"k_lbfgs<{e4}>: no FMA inside its divisions (is the division still correctly rounded?)"


def test_k_adam_arithmetic_is_the_models(disassembly):
    """k_adam, operation by operation, is what tests/adam_model.py models -- checked on the shipped code, without a GPU:

      * exactly two v_div_scale_f32 ... v_div_fixup_f32 windows: sqrt(v) / bc2s and (step_neg * m) / denom, both
        correctly rounded (fast math would turn them into v_rcp_f32 and a multiplication);
      * outside them exactly ONE fused multiply-add whose product is not negated: the lerp m + w1 * (g - m)
        (__builtin_fmaf).  A second one means a contracted v * b2 + (w2 * g) * g (-ffp-contract=off dropped), none means
        the lerp lost its FMA;
      * outside them exactly TWO v_fma_f32 with a negated first factor, both after the v_sqrt_f32: the residuals
        x - s * s' with which the compiler's correctly rounded sqrtf picks among the neighbours of the hardware estimate
        (read in the disassembly: v_sqrt_f32, two v_fma_f32 -vA, vB, vX, compares, selects, v_cmp_class_f32).  They are
        why the issue's plain "FMAs outside the divisions = the lerp" count does not fit: with fast math they vanish;
      * no v_mad_f32 / v_mac_f32.  v_fmamk_f32 / v_fmaak_f32 appear, but only with the literals 2^32 and -2^32
        (0x4f800000, 0xcf800000): the 64-bit integer division idx / per of the best-iterate row index seeds its
        reciprocal with them (v_cvt_f32_u32 in, v_cvt_u32_f32 out).  No value of the Adam arithmetic passes through."""
    found = [ops for txt in disassembly for name, ops in _function_lines(txt).items() if name == "_Z6k_adam10AdamParams"]
    assert len(found) == 1, f"k_adam found {len(found)} times in the device code"
    ops = found[0]
    names = [op for op, _ in ops]
    assert not {"v_mad_f32", "v_mac_f32"} & set(names)
    for op, args in ops:
        if op in ("v_fmamk_f32", "v_fmaak_f32"):
            assert re.search(r"\b0x[4c]f800000\b", args), f"k_adam: {op} {args} is not the integer division's 2^32 scaling"
    windows, inside, lerp, residuals, fma_inside, seen_sqrt = 0, False, [], [], 0, False
    for op, args in ops:
        if op == "v_div_scale_f32":
            inside = True
        elif op == "v_div_fixup_f32":
            assert inside, "k_adam: v_div_fixup_f32 without v_div_scale_f32"
            windows, inside = windows + 1, False
        elif op == "v_sqrt_f32":
            assert not inside
            seen_sqrt = True
        elif op in ("v_fma_f32", "v_fmac_f32"):
            if inside:
                fma_inside += 1
            elif op == "v_fma_f32" and re.match(r"v\d+, -", args):
                assert seen_sqrt, f"k_adam: negated-product FMA before the square root: {args}"
                residuals.append(args)
            else:
                lerp.append(f"{op} {args}")
    assert windows == 2, f"k_adam: {windows} division windows, expected 2 (sqrt(v) / bc2s, (step_neg * m) / denom)"
    assert fma_inside > 0 and names.count("v_sqrt_f32") == 1
    assert len(lerp) == 1, f"k_adam: fused multiply-adds outside the divisions and the square root: {lerp} (expected the lerp alone)"
    assert len(residuals) == 2, f"k_adam: square-root residuals {residuals}"
