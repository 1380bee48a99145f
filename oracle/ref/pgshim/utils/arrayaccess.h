/* utils/arrayaccess.h -- STAND-IN (see postgres.h here): element-by-element array access. */
#ifndef PGSHIM_ARRAYACCESS_H
#define PGSHIM_ARRAYACCESS_H
#include "utils/array.h"

#define AARR_NDIM(a) ARR_NDIM(a)
#define AARR_DIMS(a) ARR_DIMS(a)
#define AARR_ELEMTYPE(a) ARR_ELEMTYPE(a)

typedef struct array_iter {
  AnyArrayType* array;
} array_iter;

void array_iter_setup(array_iter* it, AnyArrayType* a);
Datum array_iter_next(array_iter* it, bool* isnull, int i, int elmlen, bool elmbyval, char elmalign);

#endif
