"""The R host (r/) cannot run here — no R in the image.  These CPU checks keep it honest as far as a
C compiler and text can: the shim compiles against declaration-only stand-ins for R's headers (tests/r_stub/ — a
syntax / prototype check that PINS NOTHING about R's behaviour), every .Call in the R sources names a registered
routine with the registered number of arguments, every library entry point the shim uses is declared in
include/chicdiff_hip.h, and the R file defines the reference's DESeq2Wrap signature."""
import hashlib
import os

import pytest
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHIM = os.path.join(ROOT, "r", "src", "chicdiff_hip_shim.c")
RSRC = [os.path.join(ROOT, "r", "R", "DESeq2Wrap_hip.R"), os.path.join(ROOT, "tools", "make_golden.R"),
        os.path.join(ROOT, "r", "R", "getFullRegionData_hip.R"), os.path.join(ROOT, "r", "R", "post_hip.R")]


def test_shim_compiles_against_declaration_only_r_headers():
    r = subprocess.run(["gcc", "-std=gnu99", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-Wno-cast-function-type",
                        "-I", os.path.join(ROOT, "tests", "r_stub"), "-I", os.path.join(ROOT, "include"), SHIM],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


def _registered():
    src = open(SHIM).read()
    reg = {m.group(1): int(m.group(2)) for m in re.finditer(r'\{"(chicdiff_hip_\w+)", \(DL_FUNC\)&\1, (\d+)\}', src)}
    # the definition of each registered routine takes that many SEXP arguments
    for name, nargs in reg.items():
        m = re.search(r"^SEXP " + name + r"\(([^)]*)\)", src, re.M | re.S)
        assert m, name
        assert m.group(1).count("SEXP") == nargs, (name, m.group(1))
    return reg


def _calls(text):
    """(.Call name, number of arguments after the name, PACKAGE excluded) for every .Call in an R source; .hipCall(name, ...)
    is the wrapper that appends PACKAGE itself."""
    out = []
    for m in re.finditer(r'\.(?:hip)?Call\("(\w+)"', text):
        i, depth, nargs, in_str = m.end(), 1, 0, None
        while depth:
            ch = text[i]
            if in_str:
                if ch == "\\":
                    i += 1
                elif ch == in_str:
                    in_str = None
            elif ch in "\"'":
                in_str = ch
            elif ch in "([{":
                depth += 1
            elif ch in ")]}":
                depth -= 1
            elif ch == "," and depth == 1:
                nargs += 1
            i += 1
        if text[m.start():].startswith(".hipCall"):
            out.append((m.group(1), nargs))
            continue
        assert "PACKAGE" in text[m.start():i]
        out.append((m.group(1), nargs - 1))  # the trailing PACKAGE = argument
    return out


def test_every_dot_call_is_registered_with_matching_arity():
    reg = _registered()
    assert len(reg) >= 18
    seen = set()
    for path in RSRC:
        if not os.path.exists(path):
            continue
        for name, nargs in _calls(open(path).read()):
            assert name in reg, (path, name)
            assert reg[name] == nargs, (path, name, nargs, reg[name])
            seen.add(name)
    for must in ("chicdiff_hip_open", "chicdiff_hip_window_sums", "chicdiff_hip_size_factors", "chicdiff_hip_theta_grid",
                 "chicdiff_hip_wald_test", "chicdiff_hip_fit", "chicdiff_hip_release", "chicdiff_hip_chinput_table",
                 "chicdiff_hip_fragment_background", "chicdiff_hip_region_universe",
                 "chicdiff_hip_ihw_apply", "chicdiff_hip_bait_flags", "chicdiff_hip_count_table", "chicdiff_hip_count_join_inner", "chicdiff_hip_count_join_multi",
                 "chicdiff_hip_region_avdist", "chicdiff_hip_download", "chicdiff_hip_upload"):
        assert must in seen, must


def test_shim_uses_only_declared_library_entry_points():
    hdr = open(os.path.join(ROOT, "include", "chicdiff_hip.h")).read()
    declared = set(re.findall(r"\b(chicdiff_hip_[a-z0-9_]+)\s*\(", hdr))
    src = open(SHIM).read()
    reg = set(_registered())
    used = set(re.findall(r"\b(chicdiff_hip_[a-z0-9_]+)\s*\(", src)) - reg
    assert used and used <= declared, used - declared
    for must in ("chicdiff_hip_window_sums_dev", "chicdiff_hip_size_factors_dev", "chicdiff_hip_offsets_dev", "chicdiff_hip_theta_grid_dev",
                 "chicdiff_hip_wald_test_dev", "chicdiff_hip_nbglm_fit_dev", "chicdiff_hip_cooks_filter_dev",
                 "chicdiff_hip_independent_filtering_dev", "chicdiff_hip_chinput_read", "chicdiff_hip_chinput_table_dev",
                 "chicdiff_hip_count_join_dev", "chicdiff_hip_fragment_background_dev", "chicdiff_hip_count_table_dev",
                 "chicdiff_hip_count_join_inner_dev", "chicdiff_hip_count_join_multi_dev", "chicdiff_hip_region_avdist_dev"):
        assert must in used, must


PATCH = os.path.join(ROOT, "r", "patches", "chicdiff_hip.patch")


def test_r_host_enters_through_the_patch_and_restates_none_of_the_reference_bodies():
    """The reference's exported functions stay the reference's: r/patches/chicdiff_hip.patch lets the device path in (one
    line at the top of getRegionUniverse / getFullRegionData, one call after DESeq2Wrap's own argument handling, the
    covariate and the application block of IHWcorrection), and r/R/ defines only what those lines call."""
    r = open(RSRC[0]).read()
    assert re.search(r'^\.DESeq2WrapHip <- function\(chicdiff\.settings, RU, FullRegionData, suffix = "", theta = NULL, norm = ', r, re.M)
    assert not re.search(r"^DESeq2Wrap <- function", r, re.M)
    for text in ("Optimising scaling factors...", "Total deviances by theta (Fullmean --> Standard):", "Theta=", "Processing model output",
                 ": # unweighted interactions with padj<0.05: ", "Standard DESeq2 normalisation",
                 "Chicago full mean-based normalisation", "combined normalisation"):
        assert text in r, text
    # the argument handling and its warnings are the reference's own statements now (the patch enters after them)
    assert "Unknown normalisation method" not in r and "Mixing parameter theta set to" not in r
    assert "unseeded" not in r and "session RNG" not in r
    g = open(RSRC[2]).read()
    assert re.search(r'^\.getFullRegionDataHip <- function\(chicdiff\.settings, RU, RUcontrol, suffix = ""\)', g, re.M)
    assert not re.search(r"^getFullRegionData <- function", g, re.M)
    p = open(RSRC[3]).read()
    assert re.search(r'^\.getRegionUniverseHip <- function\(chicdiff\.settings, suffix = ""\)', p, re.M)
    assert not re.search(r"^(IHWcorrection|getRegionUniverse) <- function", p, re.M)   # no clone of the reference's bodies
    for helper in (".isHipRegionData", ".hipRegionDistances", ".hipApplyIHWweights"):
        assert re.search(r"^" + re.escape(helper) + r" <- function", p, re.M), helper
    # every function the patch's added lines call is defined in r/R/ with the formals it is given
    patch = open(PATCH).read()
    added = [l[1:] for l in patch.splitlines() if l.startswith("+") and not l.startswith("+++")]
    removed = [l for l in patch.splitlines() if l.startswith("-") and not l.startswith("---")]
    assert len(added) <= 15 and len(removed) <= 2, (len(added), len(removed))
    texts = "\n".join(_r_strip(open(q).read()) for q in _r_host_sources())
    own = {}
    for m in re.finditer(r"(" + _NAME + r")\s*(?:<-|=)\s*function\s*\(", texts):
        formals, _ = _r_args(texts, m.end() - 1)
        own[m.group(1)] = [re.split(r"\s*=", a, maxsplit=1)[0].strip() for a in formals]
    called = set()
    for line in added:
        st = _r_strip(line)
        for m in re.finditer(r"(\.[A-Za-z][A-Za-z0-9._]*)\s*\(", st):
            name = m.group(1)
            assert name in own, f"the patch calls {name}(), which r/R/ does not define"
            called.add(name)
            args, _ = _r_args(st, m.end() - 1)
            for a in args:
                nm = re.match(r"(" + _NAME + r")\s*=(?!=)", a)
                if nm:
                    assert nm.group(1) in own[name], (name, nm.group(1), own[name])
    assert called == {".getRegionUniverseHip", ".getFullRegionDataHip", ".DESeq2WrapHip", ".isHipRegionData", ".hipRegionDistances",
                      ".hipApplyIHWweights", ".hipDeviceIndex"}, called


def _digest(line):
    """what tests/golden/reference_chicdiff_R_digests.json holds for a line of the reference (tools/make_reference_line_digests.py)"""
    return hashlib.sha256(line.encode("utf-8")).hexdigest()[:16]


def _code_lines(lines):
    """VERDICT r03's line-overlap measure: comments and whitespace stripped, package prefixes removed"""
    out = []
    for l in lines:
        l = re.sub(r"#.*$", "", l)
        l = re.sub(r"\b(data\.table|stats|IHW|cowplot|ggplot2|Chicago|DESeq2|utils|methods)::", "", l)
        l = re.sub(r"\s+", "", l)
        # not statements one could have written differently: a lone brace / `}else{`, and message() — a drop-in must emit the
        # reference's progress messages verbatim ("Side effects: messages")
        if len(l) > 3 and l != "}else{" and not l.startswith("message("):
            out.append(l)
    return out


def _hunks(patch_text):
    """(target file, [(old start, old-side lines, new-side line count)]) of a one-file unified diff"""
    lines = patch_text.split("\n")
    target, hunks, i = None, [], 0
    while i < len(lines):
        m = re.match(r"@@ -(\d+)(?:,(\d+))? \+\d+(?:,(\d+))? @@", lines[i])
        if lines[i].startswith("--- a/"):
            target = lines[i][len("--- a/"):].split("\t")[0]
        if not m:
            i += 1
            continue
        start, n_old, n_new = int(m.group(1)), int(m.group(2) or 1), int(m.group(3) or 1)
        old, new_count, i = [], 0, i + 1
        while len(old) < n_old or new_count < n_new:
            assert i < len(lines), ("hunk at", start, "ends early")
            l = lines[i]
            assert l[:1] in (" ", "-", "+", "\\"), ("hunk at", start, "malformed line", l)
            if l[:1] in (" ", "-"):
                old.append(l[1:])
            if l[:1] in (" ", "+"):
                new_count += 1
            i += 1
        assert (len(old), new_count) == (n_old, n_new), ("hunk at", start, "line counts differ from its header")
        hunks.append((start, old, new_count))
    return target, hunks


def test_patch_applies_to_the_reference_and_r_host_shares_few_lines_with_it():
    """Against the reference's Chicdiff/R/chicdiff.R as digested in tests/golden/reference_chicdiff_R_digests.json: every hunk
    of the committed patch finds its context and removed lines at the line numbers it names (what `patch` needs to apply it
    without offset or fuzz), and every file under r/R/ shares fewer than 10 code lines with the reference."""
    import json
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_chicdiff_R_digests.json")))
    target, hunks = _hunks(open(PATCH).read())
    assert target == ref["source"], (target, ref["source"])
    assert len(hunks) >= 7
    for start, old, _ in hunks:
        at = ref["lines"][start - 1:start - 1 + len(old)]
        assert [_digest(l) for l in old] == at, ("hunk at line", start, "does not match the reference there")

    ref_lines = set(ref["code_lines"])
    for path in _r_host_sources():
        mine = _code_lines(open(path, errors="replace"))
        same = [l for l in mine if _digest(l) in ref_lines]
        print(os.path.basename(path), "code lines", len(mine), "identical to a reference line:", len(same))
        assert len(same) < 10, (path, same)


# ---- a lint of the R sources: what a typo would break ---------------------------------------------------------------
# (text only — it resolves names and argument names, it does not evaluate anything)

def _r_strip(src):
    """comments out, string literals -> "" (so that brackets and names inside them do not count)"""
    out, i, n = [], 0, len(src)
    while i < n:
        c = src[i]
        if c == "#":
            while i < n and src[i] != "\n":
                i += 1
        elif c in "\"'":
            q = c
            i += 1
            while i < n and src[i] != q:
                if src[i] == "\\":
                    i += 1
                i += 1
            i += 1
            out.append('""')
        elif c == "`":
            j = src.index("`", i + 1)
            out.append(src[i:j + 1])
            i = j + 1
        else:
            out.append(c)
            i += 1
    return "".join(out)


def _r_args(s, open_paren):
    """top-level arguments of the call whose "(" is at s[open_paren]; returns (list of argument texts, index after ")")"""
    depth, cur, args, i = 0, "", [], open_paren
    while i < len(s):
        c = s[i]
        if c in "([{":
            depth += 1
            if depth > 1:
                cur += c
        elif c in ")]}":
            depth -= 1
            if depth == 0:
                args.append(cur)
                return [a.strip() for a in args if a.strip()], i + 1
            cur += c
        elif c == "," and depth == 1:
            args.append(cur)
            cur = ""
        else:
            cur += c
        i += 1
    raise AssertionError("unbalanced call")


_NAME = r"[A-Za-z.][A-Za-z0-9._]*"
# base / stats / utils functions and control-flow words the host uses: a new name must be added here deliberately
_BASE = set("""abs all any anyNA array as.character as.data.frame as.double as.integer attributes bitwAnd c cat cbind class dev.off
emptyenv factor for function getOption head identical if inherits is.na is.nan is.null lapply length list log match matrix max mean
merge message min names ncol new.env nrow numeric on.exit order paste paste0 plot rep return rowSums runif sample sapply saveRDS
seq_along seq_len setdiff sort sprintf stderr stop stopifnot storage.mode structure sum suppressWarnings table unique unlist vector
warning which while repeat switch tryCatch exp sqrt floor round is.numeric is.character nchar rev cumsum do.call Reduce Filter Map
vapply mapply file.path basename readRDS load get exists environment invisible .Call""".split())
_PKGS = {"data.table", "stats", "IHW", "cowplot", "ggplot2", "Chicago", "DESeq2", "utils", "methods"}


def _r_host_sources():
    return [p for p in RSRC if os.sep + "r" + os.sep in p]


def test_r_sources_brackets_balance():
    for path in RSRC:
        s = _r_strip(open(path).read())
        stack = []
        pairs = {")": "(", "]": "[", "}": "{"}
        for k, c in enumerate(s):
            if c in "([{":
                stack.append((c, s.count("\n", 0, k) + 1))
            elif c in ")]}":
                assert stack and stack[-1][0] == pairs[c], (path, "line", s.count("\n", 0, k) + 1, c)
                stack.pop()
        assert not stack, (path, stack[-3:])


def test_every_function_the_r_host_calls_exists_and_takes_the_arguments_it_is_given():
    """A name the host calls is one of: a function defined in r/R/ (or a parameter / local of the calling file), a function
    the reference defines (tests/golden/reference_functions.json: names and formals from Chicdiff/R/chicdiff.R, made by
    tools/make_reference_function_index.py), a pkg::name of a package the reference already imports, or a listed base function.  Named
    arguments passed to the reference's or the host's own functions are formals of those functions."""
    import json
    ref = json.load(open(os.path.join(ROOT, "tests", "golden", "reference_functions.json")))
    texts = {p: _r_strip(open(p).read()) for p in _r_host_sources()}
    own = {}
    for p, s in texts.items():
        for m in re.finditer(r"(" + _NAME + r")\s*(?:<-|=)\s*function\s*\(", s):
            formals, _ = _r_args(s, m.end() - 1)
            own[m.group(1)] = [re.split(r"\s*=", a, maxsplit=1)[0].strip() for a in formals]
    checked = 0
    for p, s in texts.items():
        params = {a for f in own.values() for a in f}
        for m in re.finditer(r"(?<![A-Za-z0-9._$@:])((?:" + _NAME + r"::)?" + _NAME + r")\s*\(", s):
            name = m.group(1)
            line = s.count("\n", 0, m.start()) + 1
            if "::" in name:
                assert name.split("::")[0] in _PKGS, (p, line, name)
                continue
            known = name in own or name in ref or name in _BASE or name in params
            assert known, f"{os.path.basename(p)}:{line}: call of unknown function {name}()"
            target = own.get(name) or (ref.get(name) if name in ref else None)
            if target is None or "..." in target:
                continue
            args, _ = _r_args(s, m.end() - 1)
            positional = 0
            for a in args:
                nm = re.match(r"(" + _NAME + r")\s*=(?!=)", a)
                if nm:
                    assert nm.group(1) in target, f"{os.path.basename(p)}:{line}: {name}() has no argument {nm.group(1)} (formals: {target})"
                else:
                    positional += 1
            assert positional <= len(target), f"{os.path.basename(p)}:{line}: {name}() takes {len(target)} arguments"
            checked += 1
    assert checked > 25  # the lint did look at calls
