"""The expand layers' fragment-ordered weight image (expand_frag in
csrc/vss_kernels.h, built by the host at vss_create): for every 16-channel
hidden chunk and every lane of the wave that owns it, the chunk's record holds
exactly the bytes the lane used to read from the layer's LDS weight image —
lds_a's 4 bf16 of a W1 / W2 row, and the float4s of the expand bias, the nine
depthwise taps and the depthwise bias.  No GPU needed.

The old reads, restated on the old LDS image's arrays (slice-local, c0 = 16 ck,
lane l = 16 g + r):
    aw[s]  = W1s[c0 + r][16 s + 4 g : +4]   bf16, s < cin / 16
    bias   = b1s[c0 + 4 g : +4]
    wk[t]  = wdws[t][c0 + 4 g : +4]         t < 9
    bb     = bdws[c0 + 4 g : +4]
    a2[cb] = W2s[16 cb + r][c0 + 4 g : +4]  bf16, cb < cout / 16
where W1s / b1s / wdws ([9][cs]) / bdws / W2s are the slice's rows / columns of
the layer's arrays.
"""
import numpy as np
import pytest

# (name, cin, chid, cout, ks): b2, b5, b7 of model/spec.json, and b7 split 4 ways (VSS_KSPLIT=1)
SHAPES = [("b2", 16, 64, 32, 1), ("b5", 48, 192, 48, 1), ("b7", 64, 256, 64, 1), ("b7_ks4", 64, 256, 64, 4)]


def _bf16_exact(rng, shape):
    a = rng.standard_normal(shape).astype(np.float32)
    return (a.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)


def _frag_off(n, i, lane):
    """Lane `lane`'s 8-B fragment i of a section of n: pairs side by side in 16 B per lane, an odd last one alone."""
    if n % 2 == 1 and i == n - 1:
        return (n // 2) * 1024 + lane * 8
    return (i // 2) * 1024 + lane * 16 + (i % 2) * 8


@pytest.mark.parametrize("name,cin,chid,cout,ks", SHAPES, ids=[s[0] for s in SHAPES])
def test_records_hold_the_lds_reads(pkg, name, cin, chid, cout, ks):
    rng = np.random.default_rng(cin * 1000 + chid + ks)
    w1, w2 = _bf16_exact(rng, (chid, cin)), _bf16_exact(rng, (cout, chid))
    b1, bdw = (rng.standard_normal(chid).astype(np.float32) for _ in range(2))
    wdw = rng.standard_normal((chid, 9)).astype(np.float32)
    nk, ncb, cs = cin // 16, cout // 16, chid // ks
    lay = pkg.expand_frag_layout(cin, cout)
    assert lay["aw"] == 0 and lay["f4s"] == 512 * nk and lay["a2"] == lay["f4s"] + 11 * 64
    assert lay["bytes"] == lay["a2"] + 512 * ncb and lay["bytes"] % 64 == 0
    for sl in range(ks):
        h0 = sl * cs
        img = pkg.expand_frag_image(w1, b1, wdw, bdw, w2, h0, cs)
        assert img.shape == (cs // 16, lay["bytes"])
        # the slice's arrays as the LDS image held them
        w1s = (w1[h0:h0 + cs].view(np.uint32) >> 16).astype(np.uint16)      # [cs][cin] bf16 bits
        w2s = (w2[:, h0:h0 + cs].view(np.uint32) >> 16).astype(np.uint16)   # [cout][cs]
        b1s, bdws, wdws = b1[h0:h0 + cs], bdw[h0:h0 + cs], np.ascontiguousarray(wdw[h0:h0 + cs].T)  # wdws [9][cs]
        covered = np.zeros(img.shape, bool)
        for ck in range(cs // 16):
            rec, c0 = img[ck], 16 * ck
            for lane in range(64):
                r, g = lane & 15, lane >> 4
                want = []  # (offset, bytes) of every read of this lane
                for s in range(nk):
                    want.append((lay["aw"] + _frag_off(nk, s, lane), w1s[c0 + r, 16 * s + 4 * g:][:4]))
                f4 = [b1s[c0 + 4 * g:][:4]] + [wdws[t, c0 + 4 * g:][:4] for t in range(9)] + [bdws[c0 + 4 * g:][:4]]
                for k, v in enumerate(f4):
                    want.append((lay["f4s"] + (4 * k + g) * 16, v))
                for cb in range(ncb):
                    want.append((lay["a2"] + _frag_off(ncb, cb, lane), w2s[16 * cb + r, c0 + 4 * g:][:4]))
                for off, v in want:
                    b = np.ascontiguousarray(v).view(np.uint8)
                    assert off % b.size == 0 and off + b.size <= lay["bytes"]
                    assert np.array_equal(rec[off:off + b.size], b), (name, sl, ck, lane, off)
                    covered[ck, off:off + b.size] = True
        assert covered.all()  # nothing else in a record: every byte is some lane's read


def test_builder_rejects_bad_slices(pkg):
    z = np.zeros
    with pytest.raises(pkg.VssError):
        pkg.expand_frag_image(z((64, 16)), z(64), z((64, 9)), z(64), z((32, 64)), 8, 16)   # h0 not a chunk
    with pytest.raises(pkg.VssError):
        pkg.expand_frag_image(z((64, 16)), z(64), z((64, 9)), z(64), z((32, 64)), 48, 32)  # past the layer
