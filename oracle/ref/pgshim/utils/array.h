/* utils/array.h -- STAND-IN (see postgres.h here): arrays as a small struct of Datums. */
#ifndef PGSHIM_ARRAY_H
#define PGSHIM_ARRAY_H
#include "fmgr.h"
#include "utils/lsyscache.h"

typedef struct ArrayType {
  Oid elemtype;
  int ndim;
  int dims[2];
  int nelems;
  Datum* elems;
} ArrayType;
typedef ArrayType AnyArrayType;

#define ARR_ELEMTYPE(a) ((a)->elemtype)
#define ARR_NDIM(a) ((a)->ndim)
#define ARR_DIMS(a) ((a)->dims)
#define DatumGetArrayTypeP(d) ((ArrayType*)DatumGetPointer(d))
#define PG_GETARG_ARRAYTYPE_P(n) DatumGetArrayTypeP(PG_GETARG_DATUM(n))
#define PG_RETURN_ARRAYTYPE_P(x) PG_RETURN_POINTER(x)

void deconstruct_array(ArrayType* array, Oid elmtype, int elmlen, bool elmbyval, char elmalign, Datum** elemsp,
                       bool** nullsp, int* nelemsp);
ArrayType* construct_md_array(Datum* elems, bool* nulls, int ndims, int* dims, int* lbs, Oid elmtype, int elmlen,
                              bool elmbyval, char elmalign);
int ArrayGetNItems(int ndim, const int* dims);

#endif
