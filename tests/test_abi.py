"""The C-ABI library loads without a GPU, exports every symbol the header declares, keeps the reference's POD layouts and
fails loudly (no CPU fallback) when no HIP device is present."""
import ctypes as C
import os
import re

import pytest

from chalkydri_amd import _abi as A
from chalkydri_amd import _lib, default_config

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _declared():
    src = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(ck_[a-z0-9_]+)\s*\(", src)))


def test_every_declared_symbol_is_exported(built):
    L = _lib.lib()
    names = _declared()
    assert len(names) >= 30
    missing = [n for n in names if not hasattr(L, n)]
    assert not missing, missing


def test_struct_layouts():
    assert C.sizeof(A.VisionMeasurement) == 64                      # crates/whacknet/src/lib.rs:92-95
    assert C.sizeof(A.ImageU8) == 24 and A.ImageU8.width.offset == 8 and A.ImageU8.stride.offset == 16   # image_u8_t
    assert C.sizeof(A.Detection) == 96 and C.sizeof(A.ClusterPoint) == 8 and C.sizeof(A.Cluster) == 16
    assert C.sizeof(A.Iso3) == 56 and C.sizeof(A.SqpnpResult) == 144
    L = _lib.lib()
    assert L.ck_abi_version() == 3


def test_defaults_mirror_the_reference(built):
    cfg = default_config(1280, 800)
    # DetectorBuilder::default + add_family_bits(tag36h11, 3) (crates/apriltags/src/lib.rs:45,230,258-262) on AprilTag-3 defaults
    assert (cfg.min_white_black_diff, cfg.max_nmaxima, cfg.refine_edges, cfg.max_hamming, cfg.n_families) == (5, 10, 1, 3, 1)
    assert abs(cfg.decode_sharpening - 0.25) < 1e-15 and abs(cfg.max_line_fit_mse - 10.0) < 1e-15
    assert cfg.families[0].contents.name == b"tag36h11"
    prm = A.SqpnpParams()
    _lib.lib().ck_sqpnp_params_default(C.byref(prm))
    assert prm.max_iter == 15 and prm.tol_sq == 1e-16               # chalkydri_sqpnp/src/lib.rs:203-204


def test_no_device_means_loud_failure(built):
    from chalkydri_amd.detector import AprilTagDetector, device_count
    if device_count() > 0:
        pytest.skip("a HIP device is present")
    with pytest.raises(_lib.ChalkydriError) as e:
        AprilTagDetector(640, 480)
    assert e.value.code == A.CK_ENODEVICE
    assert b"no CPU fallback" in _lib.lib().ck_strerror(A.CK_ENODEVICE)


def test_product_package_never_touches_the_oracle():
    """No import, link, dlopen or call of anything under oracle/ from the product (comments may cite oracle functions)."""
    pkg = os.path.join(ROOT, "chalkydri_amd")
    for dp, _, fs in os.walk(pkg):
        if os.sep + "build" in dp:
            continue
        for f in fs:
            path = os.path.join(dp, f)
            if f.endswith((".hip", ".c", ".h", ".cpp", ".hpp")):
                text = open(path, errors="ignore").read()
                code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
                code = re.sub(r"//[^\n]*", "", code)
                assert not re.search(r"\bora_[a-z0-9_]+\s*\(", code), path
                assert "ck_oracle" not in code and "oracle/" not in code, path
            elif f.endswith(".py") or f == "Makefile":
                text = open(path, errors="ignore").read()
                assert "pyoracle" not in text and "libck_oracle" not in text and "ck_oracle" not in text, path
                assert not re.search(r"^\s*(from|import)\s+oracle", text, flags=re.M), path


def test_create_validates_before_touching_a_device(built):
    """Argument errors are reported without a GPU: the order in ck_create is validation first, device second."""
    import ctypes as C
    from chalkydri_amd import _abi as A, default_config
    from chalkydri_amd.detector import _bind
    from chalkydri_amd._lib import lib
    L = _bind(lib())
    h = C.c_void_p()

    def rc(**kw):
        size = kw.pop("size", (640, 480))
        cfg = default_config(size[0], size[1], **kw)
        return L.ck_create(C.byref(cfg), C.byref(h))
    assert rc(size=(8, 8)) == A.CK_EINVAL                       # smaller than the 16-pixel minimum
    assert rc(size=(5000, 480)) == A.CK_EINVAL                  # boundary points carry 13-bit half-pixel coordinates
    assert rc(quad_decimate=3) == A.CK_EUNSUPPORTED
    assert rc(min_component_px=0) == A.CK_EINVAL
    # any image_u8_t the reference accepts (crates/apriltags/src/lib.rs:204-209) is a valid geometry: widths that are not
    # multiples of 4, heights that leave 1..3 rows for the last tile row, large component thresholds
    for kw in ({"size": (642, 480)}, {"size": (641, 450)}, {"size": (640, 450)}, {"size": (130, 33)}, {"min_component_px": 200}):
        assert rc(**kw) in (A.CK_OK, A.CK_ENODEVICE), kw
        if h.value:
            L.ck_destroy(h)
            h.value = None
    assert rc() in (A.CK_OK, A.CK_ENODEVICE)                    # a valid config fails only for lack of a device
    if h.value:
        L.ck_destroy(h)


def test_create_refuses_more_candidates_than_finalize_can_rank(built):
    """max_quads_per_frame x n_families is bounded by CK_MAX_FRAME_CANDIDATES (k_finalize's rank array in workgroup memory, 64 KiB
    without a raised limit): one more is CK_EINVAL before any device is looked for, the bound itself is accepted."""
    from chalkydri_amd.detector import _bind
    L = _bind(_lib.lib())
    h = C.c_void_p()
    src = open(os.path.join(ROOT, "include", "chalkydri_hip.h")).read()
    bound = int(re.search(r"#define\s+CK_MAX_FRAME_CANDIDATES\s+(\d+)", src).group(1))
    assert bound * 4 == 64 * 1024
    t36 = _lib.family("tag36h11")

    def rc(quads, nfam):
        cfg = default_config(64, 48, families=(t36,) * nfam, max_quads_per_frame=quads)
        r = L.ck_create(C.byref(cfg), C.byref(h))
        if h.value:
            L.ck_destroy(h)
            h.value = None
        return r
    for nfam in (1, 2, 4):
        assert rc(bound // nfam + 1, nfam) == A.CK_EINVAL, nfam
        assert rc(bound // nfam, nfam) in (A.CK_OK, A.CK_ENODEVICE), nfam
    assert rc(0x7FFFFFFF, 4) == A.CK_EINVAL                     # (the product does not wrap)
    assert rc(0, 4) in (A.CK_OK, A.CK_ENODEVICE)                # the default of 1024 quads with every family slot used


def test_create_refuses_bad_families(built):
    """ck_create checks what k_decode relies on for memory safety (ck_family_t's rules in chalkydri_hip.h): each bad table is
    CK_EINVAL before any device is looked for; the good table it was made from is accepted."""
    import sys
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import family_gen as fg
    from chalkydri_amd.detector import _bind
    L = _bind(_lib.lib())
    h = C.c_void_p()
    nbits, wab, tw, rev, cells, mh, _ = fg.MATRIX["std41r"]
    bx, by = fg.layout(cells, wab)
    codes = [int(c) for c in fg.tables(fg.make("std41r"))[6]]

    def rc(**kw):
        a = dict(nbits=nbits, wab=wab, tw=tw, rev=rev, bx=bx, by=by, codes=codes, min_hamming=mh)
        a.update(kw)
        fam = fg.family_from("bad", **a)
        cfg = default_config(640, 480, families=(_lib.family("tag36h11"), fam))
        r = L.ck_create(C.byref(cfg), C.byref(h))
        if h.value:
            L.ck_destroy(h)
            h.value = None
        return r

    assert rc() in (A.CK_OK, A.CK_ENODEVICE)
    # every bad table below breaks exactly one rule (the others hold for it), so each rule is pinned by its own case
    shift = lambda d: dict(bx=[x + d for x in bx], by=[y + d for y in by])
    assert rc(nbits=0, codes=[0]) == A.CK_EINVAL                                        # nbits >= 1
    assert rc(nbits=65, bx=bx + bx[:24], by=by + by[:24]) == A.CK_EINVAL               # nbits <= 64 (65 valid cells)
    assert rc(codes=[]) == A.CK_EINVAL                                                  # ncodes >= 1
    assert rc(codes=[codes[0]] * (1 << 20)) == A.CK_EINVAL                              # ids are 20 bits of the codebook search's key
    assert rc(codes=[codes[0]] * ((1 << 20) - 1)) in (A.CK_OK, A.CK_ENODEVICE)
    assert rc(n_upstream=len(codes) + 1) == A.CK_EINVAL                                 # n_upstream <= ncodes
    assert rc(wab=0, **shift(-2)) == A.CK_EINVAL                                        # width_at_border >= 1 (grid [-4, 5))
    assert rc(tw=17) == A.CK_EINVAL                                                     # total_width <= 16 (grid [-6, 11))
    # width_at_border <= total_width: 8 * 17 = 136 border samples would overrun k_decode's 128 (grid [0, 16))
    assert rc(wab=17, tw=16, **shift(2)) == A.CK_EINVAL
    assert rc(wab=16, tw=16, **shift(2)) in (A.CK_OK, A.CK_ENODEVICE)
    lo, hi = (wab - tw) // 2, (wab - tw) // 2 + tw                                      # every cell in the grid [lo, hi) = [-2, 7)
    assert rc(bx=[lo] + bx[1:], by=[lo] + by[1:]) in (A.CK_OK, A.CK_ENODEVICE) and rc(bx=bx[:-1] + [hi - 1]) in (A.CK_OK, A.CK_ENODEVICE)
    for i, x, y in [(0, lo - 1, None), (7, None, hi), (40, hi, None), (20, None, lo - 1), (3, 1 << 20, None)]:
        assert rc(bx=[x if (j == i and x is not None) else v for j, v in enumerate(bx)],
                  by=[y if (j == i and y is not None) else v for j, v in enumerate(by)]) == A.CK_EINVAL, i
    assert rc(codes=codes + [codes[0] | (1 << nbits)]) == A.CK_EINVAL                  # every code < 2^nbits
    # NULL tables, in a child: without the check ck_create would read through the NULL pointer, which ends the process
    import subprocess
    child = ("import sys, ctypes as C; sys.path[:0] = [{root!r}, {here!r}]\n"
             "import family_gen as fg\n"
             "from chalkydri_amd import _abi as A, _lib, default_config\n"
             "from chalkydri_amd.detector import _bind\n"
             "L, h = _bind(_lib.lib()), C.c_void_p()\n"
             "fam = fg.make('std41r')\n"
             "setattr(fam.contents, sys.argv[1], None)\n"
             "print('rc', L.ck_create(C.byref(default_config(640, 480, families=(fam,))), C.byref(h)))\n"
             ).format(root=ROOT, here=os.path.dirname(os.path.abspath(__file__)))
    for field in ("codes", "bit_x", "bit_y"):
        r = subprocess.run([sys.executable, "-c", child, field], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and f"rc {A.CK_EINVAL}" in r.stdout, (field, r.returncode, r.stdout[-500:], r.stderr[-500:])
    # the 64-bit word: every code is in range, none is refused for its top bit
    assert L.ck_create(C.byref(default_config(640, 480, families=(fg.make("full64"), fg.make("full64w")))), C.byref(h)) in (A.CK_OK, A.CK_ENODEVICE)
    if h.value:
        L.ck_destroy(h)
        h.value = None


def test_product_library_reads_no_diagnostic_knob(built):
    """The drop-in must not change what it returns with the environment: the measurement / path-forcing knobs (CK_*_STOP_AFTER,
    CK_FIT_SKIP, CK_FMERGE_CAP, CK_EXT_BASE, ...) exist only in the -DCK_DIAG build (lib/diag/).  The product library names exactly
    one variable: CK_POISON (allocation fill / guard pages)."""
    import re
    from conftest import DIAG_LIB
    from chalkydri_amd import _lib
    prod = open(os.path.join(os.path.dirname(_lib.__file__), "lib", "libchalkydri_hip.so"), "rb").read()
    names = set(m.decode() for m in re.findall(rb"CK_[A-Z0-9_]{3,}(?=\x00)", prod))
    # (error-code names appear in ck_strerror's texts; anything else that looks like a knob is a failure)
    knobs = {n for n in names if not n.startswith(("CK_E", "CK_OK", "CK_FRAME_", "CK_HIP", "CK_ALLOC", "CK_ABI"))}
    assert knobs <= {"CK_POISON"}, knobs
    assert b"STOP_AFTER" not in prod and b"CK_FIT_" not in prod and b"CK_FMERGE" not in prod and b"CK_EXT_BASE" not in prod
    assert b"k_ext_base" not in prod   # (the kernel that sets the knob's value is the diagnostics build's too)
    diag = open(DIAG_LIB, "rb").read()
    for k in (b"CK_TILE_STOP_AFTER", b"CK_FMERGE_CAP", b"CK_FIT_FLAT", b"CK_FIT_SKIP", b"CK_EMIT_STOP_AFTER", b"CK_EXT_BASE"):
        assert k in diag, k


def test_diagnostics_library_is_the_products_device_code_but_for_k_chunk(built):
    """Every path-forcing test runs against the diagnostics library (lib/diag/), so what it proves about a kernel holds for the product
    only if the kernel is the same one.  It is, by construction: that library links the product's own object files and compiles only
    ck_knobs.c and k_chunk.hip a second time (csrc/Makefile).  Here: the gfx950 code objects of the two libraries, one per unit, are
    byte for byte the same but for one on each side, and that one holds k_chunk."""
    import collections
    import hashlib
    import shutil
    import subprocess
    import tempfile
    from conftest import DIAG_LIB
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")

    def code_objects(lib):   # SHA-256 -> bytes, and the multiset of the SHA-256s
        with tempfile.TemporaryDirectory() as td:
            shutil.copy(lib, os.path.join(td, "lib.so"))
            subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", "lib.so"], cwd=td, stdout=subprocess.DEVNULL)
            blobs = [open(os.path.join(td, f), "rb").read() for f in sorted(os.listdir(td)) if f.startswith("lib.so") and "amdgcn" in f]
        by_sum = {hashlib.sha256(b).hexdigest(): b for b in blobs}
        return by_sum, collections.Counter(hashlib.sha256(b).hexdigest() for b in blobs)

    prod, n_prod = code_objects(os.path.join(os.path.dirname(_lib.__file__), "lib", "libchalkydri_hip.so"))
    diag, n_diag = code_objects(DIAG_LIB)
    assert sum(n_prod.values()) == sum(n_diag.values()) >= 20   # one per HIP unit
    only_prod, only_diag = n_prod - n_diag, n_diag - n_prod
    assert sum(only_prod.values()) == 1 and sum(only_diag.values()) == 1, (only_prod, only_diag)
    for by_sum, odd in ((prod, only_prod), (diag, only_diag)):
        assert re.search(rb"7k_chunkE\w+\.kd\x00", by_sum[next(iter(odd))])   # the kernel descriptor's symbol: (anonymous namespace)::k_chunk(...)


def test_knob_table_says_how_each_site_reads_its_knob():
    """ck_knobs.h is the one list of the diagnostic knobs.  Every row has exactly one site that reads it, and the row's ONCE / PER_CALL
    is what the site does: a `static const int` keeps the first call's value, anything else reads the environment in every call
    (the path-forcing tests change the PER_CALL ones between two calls of one process)."""
    csrc = os.path.join(ROOT, "chalkydri_amd", "csrc")
    rows = re.findall(r"^\s*X\((\w+),\s*(-?\d+), (ONCE|PER_CALL),\s*\"[^\"]+\"\)", open(os.path.join(csrc, "ck_knobs.h")).read(), re.M)
    assert len(rows) == 14 and {r[0] for r in rows if r[2] == "PER_CALL"} == {"FMERGE_CAP", "FMERGE_BAND_ROWS", "FIT_STOP_AFTER", "EXT_BASE",
                                                                           "CHUNK_STOP_AFTER"}
    lines = [l for f in os.listdir(csrc) if f.endswith(".hip") for l in open(os.path.join(csrc, f)).read().splitlines()]
    for name, _, read in rows:
        sites = [l for l in lines if "ck_knob(CK_KNOB_%s)" % name in l]
        assert len(sites) == 1 and ("static const int" in sites[0]) == (read == "ONCE"), (name, sites)


def test_fit_kernels_keep_their_register_budgets(built):
    """The split quad fit's kernels read other lanes' registers (v_readlane) around divergent code; a build of k_tail that spilled
    heavily once lost detections (the reads stood inside divergent blocks, where the spill code restores active lanes
    only).  The reads are all-lane now and the current build is verified by the full-size tests — this check makes a toolchain or
    source change that pushes a kernel over its budget fail HERE, on the CPU, instead of silently at 2448x2048: the code
    object's own metadata (llvm-readelf --notes) must show no spill in k_chunk and k_tile, at most the known 2 registers in
    k_tail, and no scratch at all in the segmentation kernels."""
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    build = os.path.join(ROOT, "chalkydri_amd", "csrc", "build")
    res = {}
    with tempfile.TemporaryDirectory() as td:
        for obj in ("k_quads.o", "k_chunk.o", "k_ccl.o"):
            shutil.copy(os.path.join(build, obj), td)
            subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", obj], cwd=td, stdout=subprocess.DEVNULL)
            co = [f for f in os.listdir(td) if f.startswith(obj) and "amdgcn" in f][0]
            notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
            name = None
            for line in notes.splitlines():
                m = re.match(r"\s*\.name:\s+(\S+)", line)
                if m:
                    name = m.group(1)
                    res[name] = {}
                m = re.match(r"\s*\.(vgpr_spill_count|sgpr_spill_count|private_segment_fixed_size|vgpr_count):\s+(\d+)", line)
                if m and name:
                    res[name][m.group(1)] = int(m.group(2))
    pick = lambda frag: [(k, v) for k, v in res.items() if frag in k]
    assert pick("k_chunk") and pick("k_tail") and pick("k_tile") and pick("k_fmerge")
    for k, v in pick("k_chunk") + pick("k_tile") + pick("k_fmerge"):
        assert v["vgpr_spill_count"] == 0 and v["private_segment_fixed_size"] == 0, (k, v)
    for k, v in pick("k_tail"):
        assert v["vgpr_spill_count"] <= 2, (k, v)
    for k, v in pick("k_seq"):   # the sort kernels: budgets as measured; a jump means the class lost its occupancy step
        assert v["vgpr_spill_count"] <= 20, (k, v)


def test_product_library_holds_one_fit_kernel_per_class(built):
    """The product code object of k_quads.o holds exactly the kernels the launch plan (k_quads.hip: FIT_CLASS) can launch: one
    k_fit and one k_seq per size class, named by their template arguments — and none that only a removed experiment reached
    (keys of the 8193..16384 class in global memory, k_seq's 2049..4096 class at two waves per EU): each costs compile time
    in both builds and can never run.  Reads the kernel names of the code object's metadata."""
    import shutil
    import subprocess
    import tempfile
    llvm = "/opt/rocm/lib/llvm/bin"
    if not os.path.exists(os.path.join(llvm, "llvm-objdump")):
        pytest.skip("no llvm-objdump in this image")
    with tempfile.TemporaryDirectory() as td:
        shutil.copy(os.path.join(ROOT, "chalkydri_amd", "csrc", "build", "k_quads.o"), td)
        subprocess.check_call([os.path.join(llvm, "llvm-objdump"), "--offloading", "k_quads.o"], cwd=td, stdout=subprocess.DEVNULL)
        co = [f for f in os.listdir(td) if f.startswith("k_quads.o") and "amdgcn" in f][0]
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", co], cwd=td, text=True)
    # Itanium names: k_fitILi64ELi512ELi64ELb1ELi3ELb0EE = k_fit<64, 512, 64, true, 3, false>
    got = {"k_fit": set(), "k_seq": set()}
    for m in re.finditer(r"\.name:\s+\S*?\d(k_fit|k_seq)I((?:L[ib]\d+E)+)E", notes):
        got[m.group(1)].add(tuple(int(x) for x in re.findall(r"L[ib](\d+)E", m.group(2))))
    # k_fit<NTH, CAP, CH, MLDS, WPS, GK>
    assert got["k_fit"] == {(64, 512, 64, 1, 3, 0), (64, 256, 64, 1, 4, 0), (128, 1024, 128, 1, 4, 0), (256, 2048, 224, 1, 4, 0),
                            (256, 4096, 512, 1, 2, 0), (512, 8192, 896, 1, 2, 0), (512, 16384, 512, 0, 2, 0),
                            (512, 65536, 896, 0, 2, 1)}, got["k_fit"]
    # k_seq<NTH, CAP, MLDS, WPS, GK>
    assert got["k_seq"] == {(64, 512, 1, 4, 0), (64, 256, 1, 4, 0), (128, 1024, 1, 4, 0), (256, 2048, 1, 4, 0), (256, 4096, 1, 3, 0),
                            (512, 8192, 1, 2, 0), (512, 16384, 0, 2, 0), (512, 65536, 0, 2, 1)}, got["k_seq"]
    assert (512, 16384, 512, 0, 4, 1) not in got["k_fit"] and (256, 4096, 1, 2, 0) not in got["k_seq"]
