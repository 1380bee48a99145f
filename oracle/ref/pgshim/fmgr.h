/* fmgr.h -- STAND-IN (see postgres.h here): the version-1 calling convention, as far as the reference uses it. */
#ifndef PGSHIM_FMGR_H
#define PGSHIM_FMGR_H
#include "postgres.h"

#define PGSHIM_MAX_ARGS 8
typedef struct FunctionCallInfoBaseData {
  void* srf_ctx;  /* the FuncCallContext of a set-returning function, NULL before its first call */
  bool srf_done;  /* set by SRF_RETURN_DONE */
  bool isnull;
  short nargs;
  Datum args[PGSHIM_MAX_ARGS];
} FunctionCallInfoBaseData;
typedef FunctionCallInfoBaseData* FunctionCallInfo;

#define PG_FUNCTION_ARGS FunctionCallInfo fcinfo
#define PG_FUNCTION_INFO_V1(name) extern Datum name(PG_FUNCTION_ARGS)
#define PG_MODULE_MAGIC extern int pgshim_module_magic

#define PG_GETARG_DATUM(n) (fcinfo->args[n])
#define PG_GETARG_INT32(n) DatumGetInt32(PG_GETARG_DATUM(n))
#define PG_GETARG_INT16(n) DatumGetInt16(PG_GETARG_DATUM(n))
#define PG_GETARG_BOOL(n) DatumGetBool(PG_GETARG_DATUM(n))
#define PG_GETARG_FLOAT4(n) DatumGetFloat4(PG_GETARG_DATUM(n))
#define PG_GETARG_POINTER(n) DatumGetPointer(PG_GETARG_DATUM(n))
#define PG_GETARG_BYTEA_P(n) DatumGetByteaP(PG_GETARG_DATUM(n))
#define PG_GETARG_TEXT_P(n) DatumGetTextP(PG_GETARG_DATUM(n))

#define PG_RETURN_DATUM(x) return (x)
#define PG_RETURN_INT32(x) return Int32GetDatum(x)
#define PG_RETURN_FLOAT4(x) return Float4GetDatum(x)
#define PG_RETURN_FLOAT8(x) return Float8GetDatum(x)
#define PG_RETURN_POINTER(x) return PointerGetDatum(x)
#define PG_RETURN_BYTEA_P(x) PG_RETURN_POINTER(x)
#define PG_RETURN_NULL()  \
  do {                    \
    fcinfo->isnull = true; \
    return (Datum)0;      \
  } while (0)

#endif
