/*
 * postgres.h -- STAND-IN, test infrastructure only.
 *
 * Declares the names of PostgreSQL's server API that the FREDDY reference sources use, written from the
 * PostgreSQL documentation ("C-Language Functions", "Server Programming Interface").  Declarations and
 * macros only; the behaviour behind them is oracle/ref/pgshim_rt.c.  The layouts are this project's own and
 * are NOT PostgreSQL's: a varlena here is a plain 4-byte length followed by the payload, an array is a
 * small struct.  The stand-ins exist so that the reference's C files can be compiled unchanged into
 * oracle/_ref/libfreddy_ref.so and run beside oracle/freddy_oracle.c on a CPU.
 */
#ifndef PGSHIM_POSTGRES_H
#define PGSHIM_POSTGRES_H

#include <math.h>
#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <sys/types.h>

typedef int16_t int16;
typedef int32_t int32;
typedef int64_t int64;
typedef uint8_t uint8;
typedef uint16_t uint16;
typedef uint32_t uint32;
typedef uint64_t uint64;
typedef float float4;
typedef double float8;
typedef unsigned int Oid;
typedef size_t Size;
typedef uintptr_t Datum;

/* variable-length datum: 4-byte total length (header included), then the payload */
struct varlena {
  int32 vl_len_;
  char vl_dat[];
};
typedef struct varlena bytea;
typedef struct varlena text;
#define VARHDRSZ ((int32)sizeof(int32))
#define VARSIZE(p) (((const struct varlena*)(p))->vl_len_)
#define VARDATA(p) (((struct varlena*)(p))->vl_dat)
#define SET_VARSIZE(p, len) (((struct varlena*)(p))->vl_len_ = (int32)(len))

/* memory */
typedef struct MemoryContextData* MemoryContext;
void* palloc(Size size);
void* palloc0(Size size);
void* repalloc(void* pointer, Size size);
void pfree(void* pointer);
MemoryContext MemoryContextSwitchTo(MemoryContext context);

/* error reporting */
#define DEBUG1 14
#define LOG 15
#define INFO 17
#define NOTICE 18
#define WARNING 19
#define ERROR 21
void elog(int elevel, const char* fmt, ...) __attribute__((format(printf, 2, 3)));
int errmsg(const char* fmt, ...) __attribute__((format(printf, 1, 2)));
int errcode(int sqlerrcode);
void pgshim_ereport_finish(int elevel);
#define ereport(elevel, rest) \
  do {                        \
    rest;                     \
    pgshim_ereport_finish(elevel); \
  } while (0)

/* Datum conversions */
float4 DatumGetFloat4(Datum d);
Datum Float4GetDatum(float4 f);
float8 DatumGetFloat8(Datum d);
Datum Float8GetDatum(float8 f);
#define DatumGetInt32(d) ((int32)(d))
#define DatumGetInt16(d) ((int16)(d))
#define DatumGetBool(d) ((bool)((d) != 0))
#define DatumGetPointer(d) ((void*)(d))
#define Int32GetDatum(x) ((Datum)(uintptr_t)(int32)(x))
#define Int16GetDatum(x) ((Datum)(uintptr_t)(int16)(x))
#define BoolGetDatum(x) ((Datum)((x) ? 1 : 0))
#define PointerGetDatum(x) ((Datum)(uintptr_t)(x))
#define DatumGetByteaP(d) ((bytea*)DatumGetPointer(d))
#define DatumGetTextP(d) ((text*)DatumGetPointer(d))

#endif
