"""numpy restatement of freddy_gpu_tokenize (include/freddy_gpu.h; freddy--0.0.1.sql:1512-1536 tokenize / tokenize_raw):
  row list    TABLE_ORDER: the distinct table rows of the ids that have one, ascending; POSITIONAL: the rows of the ids that have
              one, in the given order, duplicates kept
  centroid    core_functions.c:371-379: out[j] = 0, then for the rows i in list order out[j] = out[j] + row_i[j] / (float)n, every
              division and every addition an np.float32 operation (correctly rounded, no FMA: numpy has none)
  normalize   the oracle's vec_normalize, which test_ref_pin_cpu.py pins to the reference's vec_normalize_bytea
  n == 0      count 0 and a vector of zeros, which the normalisation leaves alone
The table is (ids ascending, vectors [N][d])."""
import numpy as np

TABLE_ORDER, POSITIONAL = 0, 1
MAX_LEN = 4096


def rows_of(table_ids, ids):
    """the table row of every id, -1 where it has none"""
    table_ids = np.asarray(table_ids, np.int64)
    ids = np.asarray(ids, np.int64).reshape(-1)
    if table_ids.size == 0:
        return np.full(ids.size, -1, np.int64)
    at = np.searchsorted(table_ids, ids)
    at_c = np.minimum(at, table_ids.size - 1)
    return np.where(table_ids[at_c] == ids, at_c, -1)


def row_list(table_ids, ids, rule):
    r = rows_of(table_ids, ids)
    r = r[r >= 0]
    return np.unique(r) if rule == TABLE_ORDER else r


def centroid(vectors, rows):
    """the reference's loop over the rows in list order"""
    d = vectors.shape[1]
    out = np.zeros(d, np.float32)
    fn = np.float32(len(rows))
    for r in rows:
        out = out + vectors[r] / fn
    assert out.dtype == np.float32
    return out


def text_vector(oracle, table_ids, vectors, ids, rule, normalize):
    rows = row_list(table_ids, ids, rule)
    v = centroid(vectors, rows)
    if normalize and len(rows):
        with np.errstate(all="ignore"):
            v = oracle.vec_normalize(v)
    return v, len(rows)


def tokenize(oracle, table_ids, vectors, texts, rule=TABLE_ORDER, normalize=True):
    """-> (vectors[n][d] float32, counts[n] int32)"""
    vectors = np.ascontiguousarray(vectors, np.float32)
    out = np.zeros((len(texts), vectors.shape[1]), np.float32)
    cnt = np.zeros(len(texts), np.int32)
    for t, ids in enumerate(texts):
        out[t], cnt[t] = text_vector(oracle, table_ids, vectors, ids, rule, normalize)
    return out, cnt
