"""Build the arithmetic mutants of the split-list composite that tests/test_gpu_split_parity.py must catch (and the older small-scale
suites, which run with splitting off, do not).  Each is one memory-safe source edit, built from a copy of csrc/ and include/:

  drop_last    the combine adds every segment's colour but the last one's
  tin          T_in(k) omits the factor of segment k-1 (the product over the segments in front stops one short)
  bwd_head_t   the backward starts every segment unit from the head's transmittance (seg_t of slot 0) instead of its own seg_t

  python scripts/split_mutations.py OUT_DIR            -> OUT_DIR/<name>/libs360.so
  python -c "import sys; sys.path[:0] = ['.', 'tests']; from splatter360_amd import _lib; from pathlib import Path; \\
      _lib.LIB_PATH = Path('OUT_DIR/tin/libs360.so'); import pytest; pytest.main(['tests/test_gpu_split_parity.py', '-m', 'gpu'])"
"""
import shutil
import sys
import tempfile
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
from splatter360_amd import _lib  # noqa: E402

MUTANTS = {
    "drop_last": ("splatter360_amd/csrc/s360_forward.hip",
                  "C01 = C01 + f2{cq[j].x, cq[j].y}; C2D = C2D + f2{cq[j].z, cq[j].w};",
                  "if (kb + j + 1u < K) { C01 = C01 + f2{cq[j].x, cq[j].y}; C2D = C2D + f2{cq[j].z, cq[j].w}; }"),
    "tin": ("splatter360_amd/csrc/s360_forward.hip",
            "for (uint32_t kk = SEG_K0; kk < k; ++kk) {", "for (uint32_t kk = SEG_K0; kk + 1u < k; ++kk) {"),
    "bwd_head_t": ("splatter360_amd/csrc/s360_bwd_em.h",
                   "pb.x = sb.seg_t[sli + lane];", "pb.x = sb.seg_t[sli - (size_t)kseg * 256u + lane];"),   # slot 0 of the same quadrant
}


def build(out_dir: Path, names=tuple(MUTANTS)) -> dict:
    built = {}
    for name in names:
        f, old, new = MUTANTS[name]
        with tempfile.TemporaryDirectory() as tmp:
            tmp = Path(tmp)
            shutil.copytree(ROOT / "splatter360_amd" / "csrc", tmp / "splatter360_amd" / "csrc")
            shutil.copytree(ROOT / "include", tmp / "include")
            src = (tmp / f).read_text()
            assert src.count(old) == 1, (name, "the mutation site moved")
            (tmp / f).write_text(src.replace(old, new))
            csrc, _lib._CSRC = _lib._CSRC, tmp / "splatter360_amd" / "csrc"
            try:
                built[name] = _lib.build(out=Path(out_dir) / name / "libs360.so")
            finally:
                _lib._CSRC = csrc
    return built


if __name__ == "__main__":
    for k, v in build(Path(sys.argv[1])).items():
        print(k, v)
