"""-m gpu, through the host-side UDF mirror (libfreddy_host.so): tokenize_batch over google_vecs_norm and tokenize_raw_batch over
google_vecs (include/freddy_udf.h) against the numpy model (tests/tokenize_model.py), bit for bit; the mirror's usual error while
google_vecs is not loaded; rows loaded in any order."""
import numpy as np
import pytest

import tokenize_inputs as ti
import tokenize_model as tm

pytestmark = pytest.mark.gpu
U = np.uint32
D = 64


def test_tokenize_batch_and_tokenize_raw_batch(oracle):
    from freddy_amd import udf
    ids, v = ti.table(D)
    raw = (v * np.float32(3.0) + np.float32(0.25)).astype(np.float32)   # google_vecs: another table under the same ids
    texts = [x for _, x in ti.texts(ids) if len(x) <= 257]
    order = np.random.default_rng(4).permutation(ids.size)
    s = udf.Session()
    try:
        with pytest.raises(udf.FreddyError, match="google_vecs_norm is not loaded"):
            s.tokenize_batch(texts, D)
        s.load_vecs_norm(ids[order], v[order])
        with pytest.raises(udf.FreddyError, match="google_vecs is not loaded"):
            s.tokenize_raw_batch(texts, D)
        s.load_vecs_original(ids[order], raw[order])
        for fn, table, normalize in ((s.tokenize_batch, v, True), (s.tokenize_raw_batch, raw, False)):
            ev, ec = tm.tokenize(oracle, ids, table, texts, tm.TABLE_ORDER, normalize)
            gv, gc = fn(texts, D)
            assert np.array_equal(gc, ec) and np.array_equal(gv.view(U), ev.view(U)), normalize
            assert (ec == 0).any() and not gv[ec == 0].any()
        gv, gc = s.tokenize_batch([], D)
        assert gv.shape == (0, D) and gc.size == 0
        with pytest.raises(udf.FreddyError, match="4097"):
            s.tokenize_batch([np.resize(ids, 4097)], D)
    finally:
        s.close()
