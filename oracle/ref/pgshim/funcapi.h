/* funcapi.h -- STAND-IN (see postgres.h here): set-returning functions and tuples built from C strings. */
#ifndef PGSHIM_FUNCAPI_H
#define PGSHIM_FUNCAPI_H
#include "fmgr.h"

typedef struct TupleDescData {
  int natts;
  Oid atttypid[8];
  char attname[8][32];
} TupleDescData;
typedef TupleDescData* TupleDesc;

/* a row: binary values for rows that SPI hands out, C strings for rows that an SRF builds */
typedef struct HeapTupleData {
  int natts;
  Datum* values;
  char** cstrings;
} HeapTupleData;
typedef HeapTupleData* HeapTuple;

typedef struct AttInMetadata {
  TupleDesc tupdesc;
} AttInMetadata;

typedef struct FuncCallContext {
  uint64 call_cntr;
  uint64 max_calls;
  void* user_fctx;
  AttInMetadata* attinmeta;
  MemoryContext multi_call_memory_ctx;
  TupleDesc tuple_desc;
} FuncCallContext;

FuncCallContext* pgshim_srf_firstcall_init(FunctionCallInfo fcinfo);
#define SRF_IS_FIRSTCALL() (fcinfo->srf_ctx == NULL)
#define SRF_FIRSTCALL_INIT() pgshim_srf_firstcall_init(fcinfo)
#define SRF_PERCALL_SETUP() ((FuncCallContext*)fcinfo->srf_ctx)
#define SRF_RETURN_NEXT(funcctx, result) \
  do {                                   \
    (funcctx)->call_cntr++;              \
    fcinfo->srf_done = false;            \
    return (result);                     \
  } while (0)
#define SRF_RETURN_DONE(funcctx) \
  do {                           \
    fcinfo->srf_done = true;     \
    return (Datum)0;             \
  } while (0)

TupleDesc CreateTemplateTupleDesc(int natts);
void TupleDescInitEntry(TupleDesc desc, int attributeNumber, const char* attributeName, Oid oidtypeid,
                        int32 typmod, int attdim);
AttInMetadata* TupleDescGetAttInMetadata(TupleDesc tupdesc);
HeapTuple BuildTupleFromCStrings(AttInMetadata* attinmeta, char** values);
Datum HeapTupleGetDatum(HeapTuple tuple);

#endif
