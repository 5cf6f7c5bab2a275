"""Generate haskoin-node_amd/csrc/hkv_mul_asm.h: 256x256 -> 512-bit product
by product scanning (column-wise) in gfx950 inline asm.

Per product: one v_mad_u64_u32 into the column's 64-bit accumulator (its
carry-out goes to an SGPR pair) and one v_addc_co_u32 that adds that carry
into the column's top word. The carry is consumed >= 2 instructions after it
is written (gfx950 VALU-writes-SGPR -> VALU-reads-SGPR spacing); three SGPR
pairs rotate. Between columns the accumulator shifts by 32 bits (C level).

The single reduced scans also get a fast form (*_fc): a column's accumulator
starts below 2^43 + 2^32, so its first full product can carry only if both
limbs lie within about 2^11 of 2^32. That product's carry-out is kept in an
SGPR pair of its own and not added; products that provably cannot carry take
no v_addc at all; after the last column the kept pairs are OR-ed into the
rare mask the form returns (ColumnBounds, fast_block, rare_or). The bounds
are computed by interval arithmetic over all-ones operands and asserted for
every column of every scan whenever the header is rendered.
    python tools/gen_mul_asm.py --schedule   (the fast forms' product order, JSON)

    python tools/gen_mul_asm.py
"""
import os

HERE = os.path.dirname(os.path.abspath(__file__))
OUT = os.path.join(HERE, "..", "haskoin-node_amd", "csrc", "hkv_mul_asm.h")


def column_block(k, pairs, name):
    """asm for one column: products `pairs` = [(i, j)], acc "+v", top "=&v"."""
    m = len(pairs)
    lines = []
    ops_in = []
    # operands: %0 acc, %1 top, %2..%4 carry pairs, then a/b regs
    regs = {}
    for (i, j) in pairs:
        for nm in (f"a{i}", f"b{j}"):
            if nm not in regs:
                regs[nm] = len(regs)
    base = 5
    ref = lambda nm: f"%{base + regs[nm]}"
    seq = []  # (kind, p)
    # schedule: mad_p at position, addc_p after mad_{p+2} (or at the end)
    for p in range(m):
        seq.append(("mad", p))
        if p - 2 >= 0:
            seq.append(("add", p - 2))
    for p in range(max(0, m - 2), m):
        seq.append(("add", p))
    emitted_mad = {}
    first_add = True
    for idx, (kind, p) in enumerate(seq):
        c = f"%{2 + p % 3}"
        if kind == "mad":
            i, j = pairs[p]
            lines.append(f"v_mad_u64_u32 %0, {c}, {ref('a%d' % i)}, {ref('b%d' % j)}, %0")
            emitted_mad[p] = len(lines) - 1
        else:
            # spacing since the mad that wrote carry p
            dist = len(lines) - 1 - emitted_mad[p]
            if dist < 2:
                lines.append(f"s_nop {1 - dist}")
            if first_add:
                lines.append(f"v_addc_co_u32_e64 %1, {c}, 0, 0, {c}")
                first_add = False
            else:
                lines.append(f"v_addc_co_u32_e64 %1, {c}, %1, 0, {c}")
    asm = "\\n\\t".join(lines)
    ins = ", ".join(f'"v"({nm[0]}[{nm[1:]}])' for nm in regs)
    return (f'  asm("{asm}"\n      : "+v"(acc), "=&v"(top), "=&s"(c0), "=&s"(c1), "=&s"(c2)\n'
            f'      : {ins});')


def scan_block(pairs, mode):
    """asm for one column of the reduced scan (mul256_red_ps / sqr256_red_ps).

    pairs: [(x, y)] C expressions of the 32-bit limb operands of the column's
    products. mode:
      "acc"  -- acc is "+v" (C-level carry-in, as in column_block)
      "red0" -- low column 0: acc = h0 * 977 (no carry-in)
      "red"  -- low column j >= 1: acc = prevhi + init, init = (top_prev << 32) | h[j-1],
                then acc += h[j] * 977. Both sums stay below 2^43, so their
                carry-outs are discarded (written to %2 before any product).
    Operands: %0 acc, %1 top, %2..%4 carry pairs; then (red modes) the prefix
    operands; then the limb operands."""
    regs = {}
    for (x, y) in pairs:
        for nm in (x, y):
            regs.setdefault(nm, len(regs))
    lines = []
    if mode == "acc":
        pre_ins = []
    elif mode in ("red0", "red0e"):
        pre_ins = ['"v"(h[0])', '"s"(k977)']
        lines.append("v_mad_u64_u32 %0, %2, %5, %6, 0")
        if mode == "red0e":  # + the addend's limb 0 (the sum stays below 2^43)
            pre_ins.append('"v"(ej)')
            lines.append("v_mad_u64_u32 %0, %2, %7, 1, %0")
    else:
        pre_ins = ['"v"(prevhi)', '"v"(init)', '"v"(hj)', '"s"(k977)']
        lines.append("v_mad_u64_u32 %0, %2, %5, 1, %6")
        lines.append("v_mad_u64_u32 %0, %2, %7, %8, %0")
        if mode == "rede":  # + the addend's limb j
            pre_ins.append('"v"(ej)')
            lines.append("v_mad_u64_u32 %0, %2, %9, 1, %0")
    base = 5 + len(pre_ins)
    ref = lambda nm: f"%{base + regs[nm]}"
    m = len(pairs)
    seq = []
    for p in range(m):
        seq.append(("mad", p))
        if p - 2 >= 0:
            seq.append(("add", p - 2))
    for p in range(max(0, m - 2), m):
        seq.append(("add", p))
    emitted_mad = {}
    first_add = True
    for kind, p in seq:
        c = f"%{2 + p % 3}"
        if kind == "mad":
            x, y = pairs[p]
            lines.append(f"v_mad_u64_u32 %0, {c}, {ref(x)}, {ref(y)}, %0")
            emitted_mad[p] = len(lines) - 1
        else:
            dist = len(lines) - 1 - emitted_mad[p]
            if dist < 2:
                lines.append(f"s_nop {1 - dist}")
            if first_add:
                lines.append(f"v_addc_co_u32_e64 %1, {c}, 0, 0, {c}")
                first_add = False
            else:
                lines.append(f"v_addc_co_u32_e64 %1, {c}, %1, 0, {c}")
    asm = "\\n\\t".join(lines)
    accc = '"+v"(acc)' if mode == "acc" else '"=&v"(accn)'
    ins = ", ".join(pre_ins + [f'"v"({nm})' for nm in regs])
    return (f'  asm("{asm}"\n      : {accc}, "=&v"(top), "=&s"(c0), "=&s"(c1), "=&s"(c2)\n'
            f'      : {ins});')


# ---------------------------------------------------------------------------
# fast forms: no carry add for a column's first product
# ---------------------------------------------------------------------------
W32 = 2**32 - 1
SEED_BOUND = 2**43            # a column's accumulator after its seeding mads
CHECK_BOUND = 2**43 + 2**32   # ... and after the products against the 1-bit limb


def op_max(nm):
    """Largest value of a limb operand: d[8] = a[7] >> 31 is one bit."""
    return 1 if nm.endswith("[8]") and nm[0] == "d" else W32


class ColumnBounds:
    """Interval arithmetic over all-ones operands for one stream of a fast
    scan: v is the largest true value (carries included) of the running
    column, so the next column's accumulator is at most v >> 32.

    classify() orders a column (products with an operand below 2^32 first) and
    gives every product its class:
      "free"   acc_max + product_max < 2^64: the mad cannot carry, no v_addc;
      "check"  the first other product, met with acc < 2^43 + 2^32: it carries
               only if the product is >= 2^64 - acc, so its carry-out goes to
               the scan's rare mask and not to top;
      "add"    every later product: one v_addc into top, as in the exact form.
    Both bounds are asserted here for every column of every scan kind."""

    def __init__(self):
        self.v = 0
        self.log = []

    def high_start(self):
        self.v >>= 32

    def low_start(self, first, addend):
        carry_in = 0 if first else (self.v >> 32) + W32   # prevhi + init, init = (top << 32) | h[j-1]
        self.v = carry_in + W32 * 977 + (W32 if addend else 0)
        assert self.v < SEED_BOUND, self.v

    def classify(self, pairs):
        order = sorted(pairs, key=lambda pr: min(op_max(pr[0]), op_max(pr[1])) == W32)
        classes, state = [], "free"
        for x, y in order:
            pm = op_max(x) * op_max(y)
            if state == "free" and self.v + pm < 2**64:
                cls = "free"
            elif state == "free" and self.v < CHECK_BOUND:
                cls, state = "check", "add"
            else:
                cls, state = "add", "add"
            self.log.append((cls, self.v, pm))
            self.v += pm
            classes.append(cls)
        return order, classes


def fast_block(pairs, classes, mode, addend, kept):
    """asm for one column of a fast scan: scan_block (three rotating carry
    pairs, a carry read two mads after its own) with the products classed by
    ColumnBounds.classify. A free product's carry pair has no reader. The
    check product writes its carry-out to a pair of its own, rk<kept>, which
    stays live to the end of the scan (rare_or): a scalar OR right behind the
    mad makes the scalar unit wait for the vector pipeline in every column
    (measured: profiles/r14_first_carry/README.md section 1).
    -> (text, the column has no v_addc: top = 0 at the C level, pairs kept so far)"""
    has_add, has_check = "add" in classes, "check" in classes
    outs = [("acc", '"+v"' if mode == "acc" else '"=&v"', "acc" if mode == "acc" else "accn")]
    if has_add:
        outs.append(("top", '"=&v"', "top"))
    outs += [(f"c{i}", '"=&s"', f"c{i}") for i in range(3)]
    if has_check:
        outs.append(("rk", '"=&s"', f"rk{kept}"))
    ins = []
    if mode == "red0":
        ins += [("h0", '"v"', "h[0]"), ("k977", '"s"', "k977")]
    elif mode == "red":
        ins += [(nm, '"v"', nm) for nm in ("prevhi", "init", "hj")] + [("k977", '"s"', "k977")]
    if addend:
        ins.append(("ej", '"v"', "ej"))
    for pr in pairs:
        for nm in pr:
            if ("L" + nm) not in [k for k, _, _ in ins]:
                ins.append(("L" + nm, '"v"', nm))
    key = {k: f"%{n}" for n, (k, _, _) in enumerate(outs + ins)}
    acc = key["acc"]
    lines = []
    if mode == "red0":
        lines.append(f"v_mad_u64_u32 {acc}, {key['c0']}, {key['h0']}, {key['k977']}, 0")
    elif mode == "red":
        lines.append(f"v_mad_u64_u32 {acc}, {key['c0']}, {key['prevhi']}, 1, {key['init']}")
        lines.append(f"v_mad_u64_u32 {acc}, {key['c0']}, {key['hj']}, {key['k977']}, {acc}")
    if addend:
        lines.append(f"v_mad_u64_u32 {acc}, {key['c0']}, {key['ej']}, 1, {acc}")
    m, seq = len(pairs), []
    for p in range(m):
        seq.append(("mad", p))
        if p - 2 >= 0:
            seq.append(("add", p - 2))
    for p in range(max(0, m - 2), m):
        seq.append(("add", p))
    emitted, first_add = {}, True
    for kind, p in seq:
        c = key["rk"] if classes[p] == "check" else key[f"c{p % 3}"]
        if kind == "mad":
            x, y = pairs[p]
            lines.append(f"v_mad_u64_u32 {acc}, {c}, {key['L' + x]}, {key['L' + y]}, {acc}")
            emitted[p] = len(lines) - 1
        elif classes[p] == "add":
            dist = len(lines) - 1 - emitted[p]
            if dist < 2:
                lines.append(f"s_nop {1 - dist}")
            lines.append(f"v_addc_co_u32_e64 {key['top']}, {c}, {'0' if first_add else key['top']}, 0, {c}")
            first_add = False
    asm = "\\n\\t".join(lines)
    text = (f'  asm("{asm}"\n      : ' + ", ".join(f"{cons}({cx})" for _, cons, cx in outs) + "\n      : " +
            ", ".join(f"{cons}({cx})" for _, cons, cx in ins) + ");")
    return text, not has_add, kept + int(has_check)


def rare_or(n):
    """The scan's rare mask: the n kept carry pairs OR-ed by the scalar unit
    after the last column. The last of them was written by column 7's first
    product, seven mads and seven v_addc before: well past the two
    instructions that a reader of a VALU-written SGPR pair keeps."""
    lines = ["s_or_b64 %0, %1, %2"] + [f"s_or_b64 %0, %0, %{j}" for j in range(3, n + 1)]
    return ('  asm("' + "\\n\\t".join(lines) + '"\n      : "=&s"(rare)\n      : ' +
            ", ".join(f'"s"(rk{j})' for j in range(n)) + '\n      : "scc");')


FAST_DOC = ["fast form: no v_addc for a column's first product. Returns the rare mask, one",
            "bit per lane whose first full product of some column carried; r and T are",
            "the exact form's whenever the mask is 0 (tools/gen_mul_asm.py ColumnBounds)."]
SCHEDULES = {}   # fast form -> [(column, [(x, y, class)])] in scan order


def fast_column(name, bounds, pairs, k, mode, addend, state):
    """One column of a fast scan: bounds, classes, asm. state: {"rare": carry
    pairs kept so far}. -> (asm text, the column's top = 0 at the C level)"""
    if mode == "acc":
        bounds.high_start()
    else:
        bounds.low_start(mode == "red0", addend)
    order, cls = bounds.classify(pairs)
    # only the first column (acc = 0, then at once near 2^64) takes a v_addc without a check before it
    assert cls.count("check") <= 1 and (k == 8 or "check" in cls or "add" not in cls), (name, k)
    SCHEDULES.setdefault(name, []).append((k, [pr + (c,) for pr, c in zip(order, cls)]))
    text, notop, state["rare"] = fast_block(order, cls, mode, addend, state["rare"])
    return text, notop


def reduced_scan(name, cols, doc, addend=False, fast=False):
    """A 256x256 product given as column pair lists cols[0..14], reduced mod p
    on the fly: columns 8..14 are scanned first (their carry-in from column 7
    is deferred), giving the high half h[0..7]; columns 0..7 then fold
    h * 2^256 == h * (2^32 + 977) into their accumulators (h[j] * 977 and
    h[j-1] enter column j). Output: r[0..7] and T < 2^38 with
    a * b == r + T * 2^256 (mod p)."""
    sig = "uint32_t r[8], uint64_t& T, const uint32_t* a, const uint32_t* b" + (", const uint32_t* e" if addend else "")
    if fast:
        exact, name, doc = name, name + "_fc", [f"{name}, " + FAST_DOC[0]] + FAST_DOC[1:]
        bounds, state = ColumnBounds(), {"rare": 0}
    out = [""] + ["// " + l for l in doc] + [
        f"__device__ __forceinline__ {'uint64_t' if fast else 'void'} {name}({sig}) {{",
        "  uint64_t acc = 0;",
        "  uint32_t top;",
        "  uint64_t c0, c1, c2" + (", rare, @RK@;" if fast else ";"),
        "  uint32_t h[8], o[8];",
        "  const uint32_t k977 = 977u;"]
    if "sqr" in name:
        out += ["  (void)b;",
                "  // row i of the square multiplies a_i by X_i = a_i + 2 * sum_{j>i} a_j 2^(32(j-i)),",
                "  // whose limbs are a_i, e[i+1] = a_{i+1} << 1, then d[i+k] = (a_{i+k} << 1) | (a_{i+k-1} >> 31)",
                "  uint32_t e[8], d[9];",
                "#pragma unroll",
                "  for (int j = 1; j < 8; ++j) e[j] = a[j] << 1;",
                "#pragma unroll",
                "  for (int j = 2; j < 8; ++j) d[j] = __builtin_amdgcn_alignbit(a[j], a[j - 1], 31);",
                "  d[8] = a[7] >> 31;"]
    for k in range(8, 15):
        out.append(f"  // column {k}: {len(cols[k])} products")
        if fast:
            blk, notop = fast_column(name, bounds, cols[k], k, "acc", False, state)
            out.append(blk)
            out += ["  top = 0;"] * notop
        else:
            out.append(scan_block(cols[k], "acc"))
        out.append(f"  h[{k - 8}] = (uint32_t)acc;")
        out.append("  acc = (acc >> 32) | ((uint64_t)top << 32);")
    out.append("  h[7] = (uint32_t)acc;  // the high half is < 2^256: nothing above")
    for j in range(8):
        out.append(f"  // column {j}: {len(cols[j])} products + h[{j}] * 977" + (f" + h[{j - 1}]" if j else ""))
        out.append("  {")
        out.append("    uint64_t accn;")
        if addend:
            out.append(f"    const uint32_t ej = e[{j}];")
        if j:
            out.append("    const uint32_t prevhi = (uint32_t)(acc >> 32);")
            out.append(f"    const uint64_t init = ((uint64_t)top << 32) | h[{j - 1}];")
            out.append(f"    const uint32_t hj = h[{j}];")
            blk = scan_block(cols[j], "rede" if addend else "red")
        else:
            blk = scan_block(cols[j], "red0e" if addend else "red0")
        if fast:
            blk, notop = fast_column(name, bounds, cols[j], j, "red" if j else "red0", addend, state)
            blk += "\n  top = 0;" * notop
        out.append("  " + blk.replace("\n", "\n  "))
        out.append("    acc = accn;")
        out.append("  }")
        out.append(f"  o[{j}] = (uint32_t)acc;")
    out.append("  T = (acc >> 32) + ((uint64_t)top << 32) + h[7];")
    out.append("  // r may alias a or b (fe_mul(x, x, y)): written only after the last column")
    out.append("#pragma unroll")
    out.append("  for (int j = 0; j < 8; ++j) r[j] = o[j];")
    out.append("  (void)c0; (void)c1; (void)c2;")
    if fast:
        assert 2 <= state["rare"] <= 14
        out.append(rare_or(state["rare"]))
        out = [l.replace("@RK@", ", ".join(f"rk{j}" for j in range(state["rare"]))) for l in out]
        out.append("  return rare;")
    out.append("}")
    return out


def reduced_functions():
    mul_cols = [[(f"a[{i}]", f"b[{k - i}]") for i in range(8) if 0 <= k - i < 8] for k in range(15)]
    sqr_cols = [[] for _ in range(16)]
    for i in range(8):
        sqr_cols[2 * i].append((f"a[{i}]", f"a[{i}]"))
        if i <= 6:
            sqr_cols[2 * i + 1].append((f"a[{i}]", f"e[{i + 1}]"))
        for j in range(i + 2, 9):
            sqr_cols[i + j].append((f"a[{i}]", f"d[{j}]"))
    assert not sqr_cols[15] and sum(map(len, sqr_cols)) == 43
    out = reduced_scan("mul256_red_ps", mul_cols, [
        "a * b mod p with the reduction folded into the product scan (HKV_MUL_RED):",
        "no separate 8-mad reduction chain, its limb moves or its two 8-limb",
        "add chains; a column's carry-in and h[j-1] enter through one mad (x 1)."])
    out += reduced_scan("mul256_red_add_ps", mul_cols, [
        "a * b + e mod p (e < 2^256): mul256_red_ps with the addend's limb j",
        "entering low column j through one more mad (x 1) — a product and an",
        "addition for one extra instruction per low column, no carry chain."], addend=True)
    out += reduced_scan("sqr256_red_ps", sqr_cols[:15], [
        "a^2 mod p as a column scan of 43 products (8 squares, 7 a_i * 2a_{i+1},",
        "28 a_i * (2a)_j limbs incl. the 1-bit limb 8) instead of 36 products plus",
        "a shift-and-add pass over 16 words, with the same folded reduction."])
    out += reduced_scan("mul256_red_ps", mul_cols, [], fast=True)
    out += reduced_scan("mul256_red_add_ps", mul_cols, [], addend=True, fast=True)
    out += reduced_scan("sqr256_red_ps", sqr_cols[:15], [], fast=True)
    return out


def reduced_sum_scan(name, sig, cols, preps, doc, fast=False):
    """A sum of two 256x256 products, a * b + c * d, given as the concatenated
    column pair lists of both terms (cols[k] = term 1's column k + term 2's),
    scanned into one set of accumulators and reduced once, as reduced_scan.

    The operands are weak form (< 2^256), so the sum is < 2^513 and the high
    half has 257 bits: after column 14 the accumulator's upper word is h[8]
    (0 or 1), and h[8] * 2^512 == h[8] * (2^32 + 977) * 2^256 enters T.
    A column takes up to 16 products; its top word counts their carries
    (<= 16), so init = (top << 32) | h[j-1] < 2^37 and the seeding sums
    prevhi + init + h[j] * 977 < 2^32 + 2^37 + 2^42 stay below 2^43 as in
    reduced_scan. T = (L + H * C) >> 256 with L < (2^36 + 15) * 2^256 (the
    low columns: 2 (k + 1) products of < 2^64 in column k) and H < 2^257,
    so T < 2^36 + 15 + 2 C + 1 < 2^37, below fe_fold_top's 2^40; the largest T,
    at all four operands 2^256 - 1, is 2^36 + 2^33 + 1935."""
    if fast:
        name, doc = name + "_fc", [f"{name}, " + FAST_DOC[0]] + FAST_DOC[1:]
        bounds, state = ColumnBounds(), {"rare": 0}
    out = [""] + ["// " + l for l in doc] + [
        f"__device__ __forceinline__ {'uint64_t' if fast else 'void'} {name}({sig}) {{",
        "  uint64_t acc = 0;",
        "  uint32_t top;",
        "  uint64_t c0, c1, c2" + (", rare, @RK@;" if fast else ";"),
        "  uint32_t h[9], o[8];",
        "  const uint32_t k977 = 977u;"]
    for pr in preps:
        out += sqr_prep(*pr)
    for k in range(8, 15):
        out.append(f"  // column {k}: {len(cols[k])} products")
        if fast:
            blk, notop = fast_column(name, bounds, cols[k], k, "acc", False, state)
            out.append(blk)
            out += ["  top = 0;"] * notop
        else:
            out.append(scan_block(cols[k], "acc"))
        out.append(f"  h[{k - 8}] = (uint32_t)acc;")
        out.append("  acc = (acc >> 32) | ((uint64_t)top << 32);")
    out.append("  const uint64_t h78 = acc;  // h[7] + h[8] * 2^32")
    out.append("  h[7] = (uint32_t)acc;")
    out.append("  h[8] = (uint32_t)(acc >> 32);  // the high half of a sum < 2^513 has 257 bits: 0 or 1")
    for j in range(8):
        out.append(f"  // column {j}: {len(cols[j])} products + h[{j}] * 977" + (f" + h[{j - 1}]" if j else ""))
        out.append("  {")
        out.append("    uint64_t accn;")
        if j:
            out.append("    const uint32_t prevhi = (uint32_t)(acc >> 32);")
            out.append(f"    const uint64_t init = ((uint64_t)top << 32) | h[{j - 1}];")
            out.append(f"    const uint32_t hj = h[{j}];")
            blk = scan_block(cols[j], "red")
        else:
            blk = scan_block(cols[j], "red0")
        if fast:
            blk, notop = fast_column(name, bounds, cols[j], j, "red" if j else "red0", False, state)
            blk += "\n  top = 0;" * notop
        out.append("  " + blk.replace("\n", "\n  "))
        out.append("    acc = accn;")
        out.append("  }")
        out.append(f"  o[{j}] = (uint32_t)acc;")
    out.append("  // T < 2^37 (see tools/gen_mul_asm.py reduced_sum_scan): h[8] * 2^512 == h[8] * (2^32 + 977) * 2^256")
    out.append("  T = ((uint64_t)h[8] * k977 + h78) + (((uint64_t)top << 32) | (acc >> 32));")
    out.append("  // r may alias any operand: written only after the last column")
    out.append("#pragma unroll")
    out.append("  for (int j = 0; j < 8; ++j) r[j] = o[j];")
    out.append("  (void)c0; (void)c1; (void)c2;")
    if fast:
        assert 2 <= state["rare"] <= 14
        out.append(rare_or(state["rare"]))
        out = [l.replace("@RK@", ", ".join(f"rk{j}" for j in range(state["rare"]))) for l in out]
        out.append("  return rare;")
    out.append("}")
    return out


def reduced_sum_functions():
    return reduced_sum_functions_(False) + reduced_sum_functions_(True)


def reduced_sum_functions_(fast):
    ab, cd = col_lists("mul", "a", "b"), col_lists("mul", "c", "d")
    aa = col_lists("sqr", "a", ("ea", "da"))
    assert max(len(x) + len(y) for x, y in zip(ab, cd)) == 16
    out = reduced_sum_scan(
        "mul256_red_sum_ps",
        "uint32_t r[8], uint64_t& T, const uint32_t* a, const uint32_t* b, const uint32_t* c, const uint32_t* d",
        [x + y for x, y in zip(ab, cd)], [],
        ["a * b + c * d mod p in one product scan (fe_mul_sum): column k sums the",
         "limb products of both terms into the same accumulators, so the two terms",
         "share one folded reduction (mul256_red_ps) and one top fold. The high half",
         "has a ninth limb h[8] (0 or 1), folded into T. Output: r[0..7] and T < 2^37",
         "with a * b + c * d == r + T * 2^256 (mod p)."], fast=fast)
    out += reduced_sum_scan(
        "sqrmul256_red_sum_ps",
        "uint32_t r[8], uint64_t& T, const uint32_t* a, const uint32_t* c, const uint32_t* d",
        [x + y for x, y in zip(aa, cd)], [("a", "ea", "da")],
        ["a^2 + c * d mod p in one product scan: the 43-product square lists of",
         "sqr256_red_ps and the 64 products of c * d, one folded reduction."], fast=fast)
    return out


def scan_block2(pairs1, pairs2, mode):
    """Two reduced-scan columns (scan_block) interleaved mad by mad, for the
    paired forms. %0 acc1, %1 top1, %2 acc2, %3 top2, %4 %5 carry pairs of
    stream 1, %6 %7 of stream 2, then the prefix operands of both streams
    (red modes), then the limb operands."""
    regs = {}
    for (x, y) in pairs1 + pairs2:
        for nm in (x, y):
            regs.setdefault(nm, len(regs))
    lines = []
    if mode == "acc":
        pre_ins = []
    elif mode == "red0":
        pre_ins = ['"v"(h1[0])', '"v"(h2[0])', '"s"(k977)']
        lines.append("v_mad_u64_u32 %0, %4, %8, %10, 0")
        lines.append("v_mad_u64_u32 %2, %6, %9, %10, 0")
    else:
        pre_ins = ['"v"(prevhi1)', '"v"(init1)', '"v"(hj1)', '"v"(prevhi2)', '"v"(init2)', '"v"(hj2)', '"s"(k977)']
        lines.append("v_mad_u64_u32 %0, %4, %8, 1, %9")
        lines.append("v_mad_u64_u32 %2, %6, %11, 1, %12")
        lines.append("v_mad_u64_u32 %0, %4, %10, %14, %0")
        lines.append("v_mad_u64_u32 %2, %6, %13, %14, %2")
    base = 8 + len(pre_ins)
    ref = lambda nm: f"%{base + regs[nm]}"
    streams = []
    for q, pairs in enumerate((pairs1, pairs2)):
        seq = []
        m = len(pairs)
        for p in range(m):
            seq.append(("mad", q, p, pairs[p]))
            if p - 1 >= 0:
                seq.append(("add", q, p - 1, None))
        if m:
            seq.append(("add", q, m - 1, None))
        streams.append(seq)
    merged = []
    for x in range(max(len(streams[0]), len(streams[1]))):
        for q in (0, 1):
            if x < len(streams[q]):
                merged.append(streams[q][x])
    emitted = {}
    first_add = [True, True]
    acc = ["%0", "%2"]
    top = ["%1", "%3"]
    for kind, q, p, pr in merged:
        c = f"%{4 + 2 * q + p % 2}"
        if kind == "mad":
            x, y = pr
            lines.append(f"v_mad_u64_u32 {acc[q]}, {c}, {ref(x)}, {ref(y)}, {acc[q]}")
            emitted[(q, p)] = len(lines) - 1
        else:
            dist = len(lines) - 1 - emitted[(q, p)]
            if dist < 2:
                lines.append(f"s_nop {1 - dist}")
            if first_add[q]:
                lines.append(f"v_addc_co_u32_e64 {top[q]}, {c}, 0, 0, {c}")
                first_add[q] = False
            else:
                lines.append(f"v_addc_co_u32_e64 {top[q]}, {c}, {top[q]}, 0, {c}")
    asm = "\\n\\t".join(lines)
    accc = '"+v"(acc1), "=&v"(top1), "+v"(acc2), "=&v"(top2)' if mode == "acc" else \
        '"=&v"(accn1), "=&v"(top1), "=&v"(accn2), "=&v"(top2)'
    ins = ", ".join(pre_ins + [f'"v"({nm})' for nm in regs])
    return (f'  asm("{asm}"\n      : {accc}, "=&s"(c0), "=&s"(c1), "=&s"(e0), "=&s"(e1)\n'
            f'      : {ins});')


def sqr_prep(src, e, d):
    return [f"  uint32_t {e}[8], {d}[9];",
            "#pragma unroll",
            f"  for (int j = 1; j < 8; ++j) {e}[j] = {src}[j] << 1;",
            "#pragma unroll",
            f"  for (int j = 2; j < 8; ++j) {d}[j] = __builtin_amdgcn_alignbit({src}[j], {src}[j - 1], 31);",
            f"  {d}[8] = {src}[7] >> 31;"]


def reduced_scan2(name, sig, cols1, cols2, preps, doc):
    out = [""] + ["// " + l for l in doc] + [
        f"__device__ __forceinline__ void {name}({sig}) {{",
        "  uint64_t acc1 = 0, acc2 = 0;",
        "  uint32_t top1, top2;",
        "  uint64_t c0, c1, e0, e1;",
        "  uint32_t h1[8], h2[8], o1[8], o2[8];",
        "  const uint32_t k977 = 977u;"]
    for pr in preps:
        out += sqr_prep(*pr)
    for k in range(8, 15):
        out.append(f"  // column {k}: {len(cols1[k])} + {len(cols2[k])} products")
        out.append(scan_block2(cols1[k], cols2[k], "acc"))
        out.append(f"  h1[{k - 8}] = (uint32_t)acc1;")
        out.append(f"  h2[{k - 8}] = (uint32_t)acc2;")
        out.append("  acc1 = (acc1 >> 32) | ((uint64_t)top1 << 32);")
        out.append("  acc2 = (acc2 >> 32) | ((uint64_t)top2 << 32);")
    out.append("  h1[7] = (uint32_t)acc1;")
    out.append("  h2[7] = (uint32_t)acc2;")
    for j in range(8):
        out.append(f"  // column {j}: {len(cols1[j])} + {len(cols2[j])} products + the folded high limbs")
        out.append("  {")
        out.append("    uint64_t accn1, accn2;")
        if j:
            for q in (1, 2):
                out.append(f"    const uint32_t prevhi{q} = (uint32_t)(acc{q} >> 32);")
                out.append(f"    const uint64_t init{q} = ((uint64_t)top{q} << 32) | h{q}[{j - 1}];")
                out.append(f"    const uint32_t hj{q} = h{q}[{j}];")
            blk = scan_block2(cols1[j], cols2[j], "red")
        else:
            blk = scan_block2(cols1[j], cols2[j], "red0")
        out.append("  " + blk.replace("\n", "\n  "))
        out.append("    acc1 = accn1;")
        out.append("    acc2 = accn2;")
        out.append("  }")
        out.append(f"  o1[{j}] = (uint32_t)acc1;")
        out.append(f"  o2[{j}] = (uint32_t)acc2;")
    out.append("  T1 = (acc1 >> 32) + ((uint64_t)top1 << 32) + h1[7];")
    out.append("  T2 = (acc2 >> 32) + ((uint64_t)top2 << 32) + h2[7];")
    out.append("#pragma unroll")
    out.append("  for (int j = 0; j < 8; ++j) { r1[j] = o1[j]; r2[j] = o2[j]; }")
    out.append("  (void)c0; (void)c1; (void)e0; (void)e1;")
    out.append("}")
    return out


def col_lists(kind, x, y=None):
    if kind == "mul":
        return [[(f"{x}[{i}]", f"{y}[{k - i}]") for i in range(8) if 0 <= k - i < 8] for k in range(15)]
    e, d = y
    cols = [[] for _ in range(16)]
    for i in range(8):
        cols[2 * i].append((f"{x}[{i}]", f"{x}[{i}]"))
        if i <= 6:
            cols[2 * i + 1].append((f"{x}[{i}]", f"{e}[{i + 1}]"))
        for j in range(i + 2, 9):
            cols[i + j].append((f"{x}[{i}]", f"{d}[{j}]"))
    return cols[:15]


def reduced_pair_functions():
    out = reduced_scan2(
        "mul256_red_ps2",
        "uint32_t r1[8], uint64_t& T1, const uint32_t* a, const uint32_t* b, uint32_t r2[8], uint64_t& T2, "
        "const uint32_t* c, const uint32_t* d",
        col_lists("mul", "a", "b"), col_lists("mul", "c", "d"), [],
        ["two independent folded-reduction products (mul256_red_ps) interleaved mad by mad"])
    out += reduced_scan2(
        "sqr256_red_ps2",
        "uint32_t r1[8], uint64_t& T1, const uint32_t* a, uint32_t r2[8], uint64_t& T2, const uint32_t* c",
        col_lists("sqr", "a", ("ea", "da")), col_lists("sqr", "c", ("ec", "dc")), [("a", "ea", "da"), ("c", "ec", "dc")],
        ["two independent folded-reduction squares (sqr256_red_ps) interleaved mad by mad"])
    out += reduced_scan2(
        "sqrmul256_red_ps2",
        "uint32_t r1[8], uint64_t& T1, const uint32_t* a, uint32_t r2[8], uint64_t& T2, const uint32_t* c, "
        "const uint32_t* d",
        col_lists("sqr", "a", ("ea", "da")), col_lists("mul", "c", "d"), [("a", "ea", "da")],
        ["a folded-reduction square beside an independent product, interleaved mad by mad"])
    return out


def render():
    """The text of hkv_mul_asm.h."""
    out = ["// GENERATED by tools/gen_mul_asm.py — do not edit.",
           "// 256x256 -> 512-bit product, product scanning in gfx950 inline asm",
           "// (one v_mad_u64_u32 per limb product and one v_addc_co_u32 for its carry; the",
           "// *_fc fast forms have no v_addc for a column's first product and return a",
           "// rare mask instead).",
           "#pragma once",
           "#include <stdint.h>",
           "",
           "namespace hkv {",
           "",
           "__device__ __forceinline__ void mul256_ps(uint32_t t[16], const uint32_t* a, const uint32_t* b) {",
           "  uint64_t acc = 0;",
           "  uint32_t top;",
           "  uint64_t c0, c1, c2;"]
    for k in range(15):
        pairs = [(i, k - i) for i in range(8) if 0 <= k - i < 8]
        out.append(f"  // column {k}: {len(pairs)} products")
        out.append(column_block(k, pairs, "mul"))
        out.append(f"  t[{k}] = (uint32_t)acc;")
        out.append("  acc = (acc >> 32) | ((uint64_t)top << 32);")
    out.append("  t[15] = (uint32_t)acc;")
    out.append("  (void)c0; (void)c1; (void)c2;")
    out.append("}")
    out.append("")
    # squaring: off-diagonal product scan, then t = 2*o + diag in one carry chain
    out.append("// 256-bit square: product scan of the 28 off-diagonal products a_i*a_j (i<j),")
    out.append("// then t = 2*o + sum a_i^2 * 2^(64 i) in one shift-and-add pass.")
    out.append("__device__ __forceinline__ void sqr256_ps(uint32_t t[16], const uint32_t* a) {")
    out.append("  const uint32_t* b = a;")
    out.append("  uint32_t o[16];")
    out.append("  uint64_t acc = 0;")
    out.append("  uint32_t top;")
    out.append("  uint64_t c0, c1, c2;")
    out.append("  o[0] = 0;")
    for k in range(1, 14):
        pairs = [(i, k - i) for i in range(8) if 0 <= k - i < 8 and i < k - i]
        out.append(f"  // column {k}: {len(pairs)} off-diagonal products")
        out.append(column_block(k, pairs, "sqr"))
        out.append(f"  o[{k}] = (uint32_t)acc;")
        out.append("  acc = (acc >> 32) | ((uint64_t)top << 32);")
    out.append("  o[14] = (uint32_t)acc;")
    out.append("  o[15] = (uint32_t)(acc >> 32);")
    out.append("  (void)c0; (void)c1; (void)c2;")
    out.append("  // t = 2*o + diagonal squares (d_{2i}, d_{2i+1}) = a_i^2")
    out.append("  uint32_t cy = 0, d0, d1;")
    out.append("#pragma unroll")
    out.append("  for (int i = 0; i < 8; ++i) {")
    out.append("    const uint64_t d = (uint64_t)a[i] * a[i];")
    out.append("    d0 = (uint32_t)d;")
    out.append("    d1 = (uint32_t)(d >> 32);")
    out.append("    const uint32_t s0 = (i == 0) ? (o[0] << 1) : __builtin_amdgcn_alignbit(o[2 * i], o[2 * i - 1], 31);")
    out.append("    const uint32_t s1 = __builtin_amdgcn_alignbit(o[2 * i + 1], o[2 * i], 31);")
    out.append("    t[2 * i] = __builtin_addc(s0, d0, cy, &cy);")
    out.append("    t[2 * i + 1] = __builtin_addc(s1, d1, cy, &cy);")
    out.append("  }")
    out.append("}")
    out.extend(reduced_functions())
    out.extend(reduced_pair_functions())
    out.extend(reduced_sum_functions())
    out.append("")
    out.append("}  // namespace hkv")
    return "\n".join(out) + "\n"


def fast_schedules():
    """The fast forms' product order as data: {name: [(column, [(x, y, class)])]
    in scan order} (tests/first_carry_model.py walks it)."""
    SCHEDULES.clear()
    render()
    return {k: list(v) for k, v in SCHEDULES.items()}


def main():
    import sys
    if sys.argv[1:] == ["--schedule"]:
        import json
        print(json.dumps(fast_schedules(), indent=1))
        return
    open(OUT, "w").write(render())
    print("wrote", OUT)


if __name__ == "__main__":
    main()
