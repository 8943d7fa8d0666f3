"""Print the ds_read_b64_tr_b16 lane map the GPU actually delivers.

Runs ``_C.lds_tr16_selftest()`` (ops/csrc/wgrad_tr.hip): a [32][64] LDS
image holding row*64+col is read as the 16x16x32 MFMA operand of each
16-column block — two transposed reads per lane, lane 4q+p of a 16-lane
group naming row q, columns 4p..4p+3 — and the 8 values per lane come back.
Expected: lane l, element j = image[k = 8*(l>>4) + j][m = 16*cb + (l&15)].

An earlier version of this probe compiled its own code object and launched
it through ctypes with a hand-packed argument buffer; it reported zeros
because of that launch path and of address patterns that were not the
instruction's contract, not because of the instruction.

python tools/tr_probe.py [column-block 0..3]
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from real_time_helmet_detection_amd.ops import _backend  # noqa: E402


def main():
    cb = int(sys.argv[1]) if len(sys.argv) > 1 else 0
    got = _backend.require_ext().lds_tr16_selftest().cpu()
    bad = 0
    for lane in range(64):
        row = got[cb, lane].tolist()
        want = [(8 * (lane >> 4) + j) * 64 + 16 * cb + (lane & 15)
                for j in range(8)]
        flag = '' if row == want else '   <-- expected %s' % want
        bad += row != want
        print('lane %2d: %s%s' % (
            lane, ' '.join('(k%2d,m%2d)' % (v // 64, v % 64) for v in row),
            flag))
    print('lane map %s' % ('OK' if not bad else 'WRONG on %d lanes' % bad))
    return 1 if bad else 0


if __name__ == '__main__':
    sys.exit(main())
