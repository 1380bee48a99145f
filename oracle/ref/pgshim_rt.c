/*
 * pgshim_rt.c -- the runtime behind oracle/ref/pgshim/: just enough of PostgreSQL's server API for the
 * FREDDY reference's C files to run on a CPU, beside oracle/freddy_oracle.c, in the test suite.
 *
 *   memory   palloc / palloc0 / repalloc / pfree over calloc, every block on one list that the driver frees
 *            after each entry point (MemoryContextSwitchTo is a no-op).
 *   errors   elog / ereport drop everything below ERROR; ERROR records the message and longjmps to the
 *            driver's trap.  Without an armed trap it prints and abort()s: a reference function that raises
 *            outside an entry point is a bug of the driver.
 *   fmgr     set-returning functions keep their FuncCallContext in fcinfo; BuildTupleFromCStrings records
 *            the row's strings.
 *   SPI      tables registered by the driver; SPI_exec accepts
 *              SELECT <cols | *> FROM <table> [AS <alias>] [WHERE <col> IN (<ints>)] [ORDER BY <col> [ASC]]
 *            where <table> may be a registered "function()" with one row.  Rows come back in stored order
 *            unless ordered (then a stable sort).  Anything else is an ERROR that names the statement.
 *
 * Written for this project from the PostgreSQL documentation's description of these interfaces.
 */
#include "pgshim_rt.h"

#include <ctype.h>
#include <stdarg.h>

#include "catalog/pg_type.h"
#include "utils/arrayaccess.h"

/* ---- errors -------------------------------------------------------------------------------------------- */
jmp_buf pgshim_error_jmp;
int pgshim_error_armed = 0;
static char error_text[512];
static char ereport_text[512];

const char* pgshim_last_error(void) { return error_text; }

static void raise_error(void) {
  if (!pgshim_error_armed) {
    fprintf(stderr, "pgshim: ERROR outside a trapped entry point: %s\n", error_text);
    abort();
  }
  pgshim_error_armed = 0;
  longjmp(pgshim_error_jmp, 1);
}

void elog(int elevel, const char* fmt, ...) {
  if (elevel < ERROR) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(error_text, sizeof error_text, fmt, ap);
  va_end(ap);
  raise_error();
}

int errmsg(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(ereport_text, sizeof ereport_text, fmt, ap);
  va_end(ap);
  return 0;
}

int errcode(int sqlerrcode) { return 0; }

void pgshim_ereport_finish(int elevel) {
  if (elevel < ERROR) return;
  snprintf(error_text, sizeof error_text, "%s", ereport_text);
  raise_error();
}

/* ---- memory -------------------------------------------------------------------------------------------- */
typedef struct block {
  struct block* prev;
  struct block* next;
  Size size;
  Size pad_;  /* keeps the payload 16-byte aligned */
} block;
static block* arena = NULL;
static long statements = 0;

static void* block_new(Size size) {
  block* b = (block*)calloc(1, sizeof(block) + (size ? size : 1));
  if (!b) {
    snprintf(error_text, sizeof error_text, "out of memory (%zu bytes)", (size_t)size);
    raise_error();
  }
  b->size = size;
  b->next = arena;
  if (arena) arena->prev = b;
  arena = b;
  return b + 1;
}

static void block_unlink(block* b) {
  if (b->prev) b->prev->next = b->next; else arena = b->next;
  if (b->next) b->next->prev = b->prev;
}

void* palloc(Size size) { return block_new(size); }
void* palloc0(Size size) { return block_new(size); }
void* SPI_palloc(Size size) { return block_new(size); }

void pfree(void* pointer) {
  if (!pointer) return;
  block* b = (block*)pointer - 1;
  block_unlink(b);
  free(b);
}

void* repalloc(void* pointer, Size size) {
  if (!pointer) return block_new(size);
  block* b = (block*)pointer - 1;
  void* fresh = block_new(size);
  memcpy(fresh, pointer, b->size < size ? b->size : size);
  pfree(pointer);
  return fresh;
}

MemoryContext MemoryContextSwitchTo(MemoryContext context) { return context; }

void pgshim_reset_memory(void) {
  while (arena) {
    block* b = arena;
    arena = b->next;
    free(b);
  }
  statements = 0;
  SPI_tuptable = NULL;
  SPI_processed = 0;
}

long pgshim_statement_count(void) { return statements; }

/* ---- Datum --------------------------------------------------------------------------------------------- */
float4 DatumGetFloat4(Datum d) {
  uint32 bits = (uint32)d;
  float4 f;
  memcpy(&f, &bits, sizeof f);
  return f;
}
Datum Float4GetDatum(float4 f) {
  uint32 bits;
  memcpy(&bits, &f, sizeof bits);
  return (Datum)bits;
}
float8 DatumGetFloat8(Datum d) {
  uint64 bits = (uint64)d;
  float8 f;
  memcpy(&f, &bits, sizeof f);
  return f;
}
Datum Float8GetDatum(float8 f) {
  uint64 bits;
  memcpy(&bits, &f, sizeof bits);
  return (Datum)bits;
}

bytea* pgshim_make_bytea(const void* data, int bytes) {
  bytea* b = (bytea*)palloc(VARHDRSZ + (Size)bytes);
  SET_VARSIZE(b, VARHDRSZ + bytes);
  if (bytes) memcpy(VARDATA(b), data, (size_t)bytes);
  return b;
}

/* ---- arrays -------------------------------------------------------------------------------------------- */
void get_typlenbyvalalign(Oid typid, int16* typlen, bool* typbyval, char* typalign) {
  switch (typid) {
    case INT2OID: *typlen = 2; *typbyval = true; *typalign = 's'; break;
    case INT4OID: *typlen = 4; *typbyval = true; *typalign = 'i'; break;
    case FLOAT4OID: *typlen = 4; *typbyval = true; *typalign = 'i'; break;
    case FLOAT8OID: *typlen = 8; *typbyval = true; *typalign = 'd'; break;
    case BYTEAOID: case TEXTOID: *typlen = -1; *typbyval = false; *typalign = 'i'; break;
    default: elog(ERROR, "pgshim: get_typlenbyvalalign: unknown type %u", typid);
  }
}

void deconstruct_array(ArrayType* array, Oid elmtype, int elmlen, bool elmbyval, char elmalign, Datum** elemsp,
                       bool** nullsp, int* nelemsp) {
  if (elmtype != array->elemtype) elog(ERROR, "pgshim: deconstruct_array: element type %u, array holds %u", elmtype, array->elemtype);
  *elemsp = (Datum*)palloc(sizeof(Datum) * (Size)array->nelems);
  if (array->nelems) memcpy(*elemsp, array->elems, sizeof(Datum) * (size_t)array->nelems);
  if (nullsp) *nullsp = (bool*)palloc0(sizeof(bool) * (Size)array->nelems);
  *nelemsp = array->nelems;
}

int ArrayGetNItems(int ndim, const int* dims) {
  if (ndim <= 0) return 0;
  int n = 1;
  for (int i = 0; i < ndim; i++) n *= dims[i];
  return n;
}

ArrayType* construct_md_array(Datum* elems, bool* nulls, int ndims, int* dims, int* lbs, Oid elmtype, int elmlen,
                              bool elmbyval, char elmalign) {
  if (ndims < 1 || ndims > 2) elog(ERROR, "pgshim: construct_md_array: %d dimensions", ndims);
  ArrayType* a = (ArrayType*)palloc0(sizeof(ArrayType));
  a->elemtype = elmtype;
  a->ndim = ndims;
  for (int i = 0; i < ndims; i++) a->dims[i] = dims[i];
  a->nelems = ArrayGetNItems(ndims, dims);
  a->elems = (Datum*)palloc(sizeof(Datum) * (Size)a->nelems);
  if (a->nelems) memcpy(a->elems, elems, sizeof(Datum) * (size_t)a->nelems);
  return a;
}

ArrayType* pgshim_make_int4_array(const int32* values, int n) {
  ArrayType* a = (ArrayType*)palloc0(sizeof(ArrayType));
  a->elemtype = INT4OID;
  a->ndim = 1;
  a->dims[0] = n;
  a->nelems = n;
  a->elems = (Datum*)palloc(sizeof(Datum) * (Size)n);
  for (int i = 0; i < n; i++) a->elems[i] = Int32GetDatum(values[i]);
  return a;
}

void array_iter_setup(array_iter* it, AnyArrayType* a) { it->array = a; }

Datum array_iter_next(array_iter* it, bool* isnull, int i, int elmlen, bool elmbyval, char elmalign) {
  if (i < 0 || i >= it->array->nelems) elog(ERROR, "pgshim: array_iter_next: element %d of %d", i, it->array->nelems);
  *isnull = false;
  return it->array->elems[i];
}

/* ---- fmgr / SRF ---------------------------------------------------------------------------------------- */
FuncCallContext* pgshim_srf_firstcall_init(FunctionCallInfo fcinfo) {
  FuncCallContext* c = (FuncCallContext*)palloc0(sizeof(FuncCallContext));
  fcinfo->srf_ctx = c;
  return c;
}

TupleDesc CreateTemplateTupleDesc(int natts) {
  if (natts < 0 || natts > 8) elog(ERROR, "pgshim: CreateTemplateTupleDesc: %d attributes", natts);
  TupleDesc d = (TupleDesc)palloc0(sizeof(TupleDescData));
  d->natts = natts;
  return d;
}

void TupleDescInitEntry(TupleDesc desc, int attributeNumber, const char* attributeName, Oid oidtypeid, int32 typmod,
                        int attdim) {
  if (attributeNumber < 1 || attributeNumber > desc->natts) elog(ERROR, "pgshim: TupleDescInitEntry: attribute %d of %d", attributeNumber, desc->natts);
  desc->atttypid[attributeNumber - 1] = oidtypeid;
  snprintf(desc->attname[attributeNumber - 1], sizeof desc->attname[0], "%s", attributeName);
}

AttInMetadata* TupleDescGetAttInMetadata(TupleDesc tupdesc) {
  AttInMetadata* m = (AttInMetadata*)palloc0(sizeof(AttInMetadata));
  m->tupdesc = tupdesc;
  return m;
}

HeapTuple BuildTupleFromCStrings(AttInMetadata* attinmeta, char** values) {
  int n = attinmeta->tupdesc->natts;
  HeapTuple t = (HeapTuple)palloc0(sizeof(HeapTupleData));
  t->natts = n;
  t->cstrings = (char**)palloc0(sizeof(char*) * (Size)n);
  for (int i = 0; i < n; i++) {
    size_t len = strlen(values[i]);
    t->cstrings[i] = (char*)palloc(len + 1);
    memcpy(t->cstrings[i], values[i], len + 1);
  }
  return t;
}

Datum HeapTupleGetDatum(HeapTuple tuple) { return PointerGetDatum(tuple); }

/* ---- tables -------------------------------------------------------------------------------------------- */
#define MAX_COLS 8
struct pgshim_table {
  char name[96];
  int ncols;
  char colname[MAX_COLS][32];
  int coltype[MAX_COLS];
  int64 nrows, cap;
  Datum* cells;  /* [nrows][ncols]; bytea / text cells own a malloc'd copy */
  struct pgshim_table* next;
};
static pgshim_table* tables = NULL;

void pgshim_drop_tables(void) {
  while (tables) {
    pgshim_table* t = tables;
    tables = t->next;
    for (int64 r = 0; r < t->nrows; r++)
      for (int c = 0; c < t->ncols; c++)
        if (t->coltype[c] == PGSHIM_BYTEA || t->coltype[c] == PGSHIM_TEXT) free(DatumGetPointer(t->cells[r * t->ncols + c]));
    free(t->cells);
    free(t);
  }
}

pgshim_table* pgshim_create_table(const char* name, int ncols, const char* const* colnames, const int* coltypes) {
  if (ncols < 1 || ncols > MAX_COLS) return NULL;
  pgshim_table* t = (pgshim_table*)calloc(1, sizeof *t);
  if (!t) return NULL;
  snprintf(t->name, sizeof t->name, "%s", name);
  t->ncols = ncols;
  for (int c = 0; c < ncols; c++) {
    snprintf(t->colname[c], sizeof t->colname[c], "%s", colnames[c]);
    t->coltype[c] = coltypes[c];
  }
  t->next = tables;
  tables = t;
  return t;
}

void pgshim_add_row(pgshim_table* t, const Datum* cells, const int* bytea_bytes) {
  if (t->nrows == t->cap) {
    t->cap = t->cap ? 2 * t->cap : 64;
    t->cells = (Datum*)realloc(t->cells, sizeof(Datum) * (size_t)t->cap * (size_t)t->ncols);
    if (!t->cells) abort();
  }
  Datum* row = t->cells + t->nrows * t->ncols;
  for (int c = 0; c < t->ncols; c++) {
    if (t->coltype[c] == PGSHIM_BYTEA) {
      int bytes = bytea_bytes[c];
      bytea* b = (bytea*)malloc((size_t)VARHDRSZ + (size_t)bytes + 1);
      if (!b) abort();
      SET_VARSIZE(b, VARHDRSZ + bytes);
      if (bytes) memcpy(VARDATA(b), DatumGetPointer(cells[c]), (size_t)bytes);
      row[c] = PointerGetDatum(b);
    } else if (t->coltype[c] == PGSHIM_TEXT) {
      const char* s = (const char*)DatumGetPointer(cells[c]);
      char* copy = (char*)malloc(strlen(s) + 1);
      if (!copy) abort();
      strcpy(copy, s);
      row[c] = PointerGetDatum(copy);
    } else {
      row[c] = cells[c];
    }
  }
  t->nrows++;
}

static pgshim_table* find_table(const char* name, size_t len) {
  for (pgshim_table* t = tables; t; t = t->next)
    if (strlen(t->name) == len && memcmp(t->name, name, len) == 0) return t;
  return NULL;
}

static int find_col(const pgshim_table* t, const char* name, size_t len) {
  for (int c = 0; c < t->ncols; c++)
    if (strlen(t->colname[c]) == len && memcmp(t->colname[c], name, len) == 0) return c;
  return -1;
}

/* ---- SPI ----------------------------------------------------------------------------------------------- */
uint64 SPI_processed = 0;
SPITupleTable* SPI_tuptable = NULL;
#define STATEMENT_LIMIT 20000

int SPI_connect(void) { return SPI_OK_CONNECT; }
int SPI_finish(void) { return SPI_OK_FINISH; }

static const char* skip_ws(const char* p) {
  while (*p == ' ') p++;
  return p;
}

/* case-sensitive keyword followed by a non-identifier character */
static int keyword(const char** pp, const char* kw) {
  const char* p = skip_ws(*pp);
  size_t n = strlen(kw);
  if (strncmp(p, kw, n) != 0) return 0;
  if (isalnum((unsigned char)p[n]) || p[n] == '_') return 0;
  *pp = p + n;
  return 1;
}

/* an identifier, optionally "qualifier.identifier" (the qualifier is dropped) and, for tables, a trailing "()" */
static int identifier(const char** pp, const char** start, size_t* len, int allow_call) {
  const char* p = skip_ws(*pp);
  const char* s = p;
  while (isalnum((unsigned char)*p) || *p == '_') p++;
  if (*p == '.' && p > s) {
    p++;
    s = p;
    while (isalnum((unsigned char)*p) || *p == '_') p++;
  }
  if (p == s) return 0;
  if (allow_call && p[0] == '(' && p[1] == ')') p += 2;
  *start = s;
  *len = (size_t)(p - s);
  *pp = p;
  return 1;
}

static int cmp_int32(const void* a, const void* b) {
  int32 x = *(const int32*)a, y = *(const int32*)b;
  return (x > y) - (x < y);
}

typedef struct sort_key {
  int32 key;
  int64 row;
} sort_key;

static int cmp_sort_key(const void* a, const void* b) {
  const sort_key* x = (const sort_key*)a;
  const sort_key* y = (const sort_key*)b;
  if (x->key != y->key) return (x->key > y->key) - (x->key < y->key);
  return (x->row > y->row) - (x->row < y->row);  /* stored order among equal keys */
}

static void bad_statement(const char* command, const char* why) {
  elog(ERROR, "pgshim: SPI cannot run this statement (%s): %.300s", why, command);
}

int SPI_exec(const char* command, long count) {
  if (++statements > STATEMENT_LIMIT) elog(ERROR, "pgshim: more than %d statements in one call: %.200s", STATEMENT_LIMIT, command);
  SPI_tuptable = NULL;
  SPI_processed = 0;
  const char* p = command;
  if (!keyword(&p, "SELECT")) bad_statement(command, "not a SELECT");

  /* column list */
  const char* colstart[MAX_COLS];
  size_t collen[MAX_COLS];
  int ncols = 0, star = 0;
  p = skip_ws(p);
  if (*p == '*') {
    star = 1;
    p++;
  } else {
    for (;;) {
      if (ncols == MAX_COLS) bad_statement(command, "too many columns");
      if (!identifier(&p, &colstart[ncols], &collen[ncols], 0)) bad_statement(command, "column name expected");
      ncols++;
      p = skip_ws(p);
      if (*p != ',') break;
      p++;
    }
  }
  if (!keyword(&p, "FROM")) bad_statement(command, "FROM expected");
  const char* tstart;
  size_t tlen;
  if (!identifier(&p, &tstart, &tlen, 1)) bad_statement(command, "table name expected");
  pgshim_table* t = find_table(tstart, tlen);
  if (!t) bad_statement(command, "no such table");
  if (keyword(&p, "AS")) {
    const char* a;
    size_t alen;
    if (!identifier(&p, &a, &alen, 0)) bad_statement(command, "alias expected");
  }
  int cols[MAX_COLS];
  if (star) {
    ncols = t->ncols;
    for (int c = 0; c < ncols; c++) cols[c] = c;
  } else {
    for (int c = 0; c < ncols; c++) {
      cols[c] = find_col(t, colstart[c], collen[c]);
      if (cols[c] < 0) bad_statement(command, "no such column");
    }
  }

  /* WHERE <col> IN (<ints>) */
  int where_col = -1;
  int32* in_list = NULL;
  int n_in = 0;
  if (keyword(&p, "WHERE")) {
    const char* c;
    size_t clen;
    if (!identifier(&p, &c, &clen, 0)) bad_statement(command, "column expected after WHERE");
    where_col = find_col(t, c, clen);
    if (where_col < 0 || t->coltype[where_col] != PGSHIM_INT4) bad_statement(command, "WHERE needs an integer column");
    if (!keyword(&p, "IN")) bad_statement(command, "IN expected");
    p = skip_ws(p);
    if (*p != '(') bad_statement(command, "( expected");
    p++;
    in_list = (int32*)palloc(sizeof(int32) * (strlen(p) / 2 + 1));
    for (;;) {
      p = skip_ws(p);
      char* end;
      long v = strtol(p, &end, 10);
      if (end == p) bad_statement(command, "integer expected in the IN list");
      in_list[n_in++] = (int32)v;
      p = skip_ws(end);
      if (*p == ',') {
        p++;
        continue;
      }
      if (*p == ')') {
        p++;
        break;
      }
      bad_statement(command, ", or ) expected in the IN list");
    }
    qsort(in_list, (size_t)n_in, sizeof(int32), cmp_int32);
  }

  /* ORDER BY <col> [ASC] */
  int order_col = -1;
  if (keyword(&p, "ORDER")) {
    if (!keyword(&p, "BY")) bad_statement(command, "BY expected");
    const char* c;
    size_t clen;
    if (!identifier(&p, &c, &clen, 0)) bad_statement(command, "column expected after ORDER BY");
    order_col = find_col(t, c, clen);
    if (order_col < 0 || t->coltype[order_col] != PGSHIM_INT4) bad_statement(command, "ORDER BY needs an integer column");
    keyword(&p, "ASC");
  }
  p = skip_ws(p);
  if (*p == ';') p = skip_ws(p + 1);
  if (*p) bad_statement(command, "trailing text");

  /* select */
  sort_key* picked = (sort_key*)palloc(sizeof(sort_key) * (Size)(t->nrows ? t->nrows : 1));
  int64 n = 0;
  for (int64 r = 0; r < t->nrows; r++) {
    if (where_col >= 0) {
      int32 v = DatumGetInt32(t->cells[r * t->ncols + where_col]);
      if (!bsearch(&v, in_list, (size_t)n_in, sizeof(int32), cmp_int32)) continue;
    }
    picked[n].row = r;
    picked[n].key = order_col >= 0 ? DatumGetInt32(t->cells[r * t->ncols + order_col]) : 0;
    n++;
  }
  if (order_col >= 0) qsort(picked, (size_t)n, sizeof(sort_key), cmp_sort_key);
  if (count > 0 && n > count) n = count;

  SPITupleTable* tt = (SPITupleTable*)palloc0(sizeof(SPITupleTable));
  tt->tupdesc = CreateTemplateTupleDesc(ncols);
  static const Oid type_oid[] = {INT4OID, FLOAT4OID, BYTEAOID, TEXTOID};
  for (int c = 0; c < ncols; c++) TupleDescInitEntry(tt->tupdesc, c + 1, t->colname[cols[c]], type_oid[t->coltype[cols[c]]], -1, 0);
  tt->vals = (HeapTuple*)palloc(sizeof(HeapTuple) * (Size)(n ? n : 1));
  HeapTupleData* rows = (HeapTupleData*)palloc0(sizeof(HeapTupleData) * (Size)(n ? n : 1));
  Datum* values = (Datum*)palloc(sizeof(Datum) * (Size)(n ? n : 1) * (Size)ncols);
  for (int64 i = 0; i < n; i++) {
    rows[i].natts = ncols;
    rows[i].values = values + i * ncols;
    for (int c = 0; c < ncols; c++) rows[i].values[c] = t->cells[picked[i].row * t->ncols + cols[c]];
    tt->vals[i] = &rows[i];
  }
  tt->numvals = (uint64)n;
  SPI_tuptable = tt;
  SPI_processed = (uint64)n;
  if (in_list) pfree(in_list);
  pfree(picked);
  return SPI_OK_SELECT;
}

int SPI_execute(const char* command, bool read_only, long count) { return SPI_exec(command, count); }

Datum SPI_getbinval(HeapTuple row, TupleDesc rowdesc, int colnumber, bool* isnull) {
  if (colnumber < 1 || colnumber > row->natts || !row->values) elog(ERROR, "pgshim: SPI_getbinval: column %d of %d", colnumber, row->natts);
  if (isnull) *isnull = false;
  return row->values[colnumber - 1];
}

char* SPI_getvalue(HeapTuple row, TupleDesc rowdesc, int colnumber) {
  if (colnumber < 1 || colnumber > row->natts || !row->values) elog(ERROR, "pgshim: SPI_getvalue: column %d of %d", colnumber, row->natts);
  Datum v = row->values[colnumber - 1];
  char* out;
  switch (rowdesc->atttypid[colnumber - 1]) {
    case TEXTOID: {
      const char* s = (const char*)DatumGetPointer(v);
      out = (char*)palloc(strlen(s) + 1);
      strcpy(out, s);
      return out;
    }
    case INT4OID:
      out = (char*)palloc(16);
      snprintf(out, 16, "%d", DatumGetInt32(v));
      return out;
    default:
      elog(ERROR, "pgshim: SPI_getvalue: column %d has no text form here", colnumber);
  }
  return NULL;
}
