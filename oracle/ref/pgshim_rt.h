/*
 * pgshim_rt.h -- what the driver (ref_driver.c) sees of the stand-in runtime: the arena, the error trap and
 * the in-memory tables behind SPI.  Test infrastructure only, CPU only.
 */
#ifndef PGSHIM_RT_H
#define PGSHIM_RT_H

#include <setjmp.h>

#include "executor/spi.h"
#include "utils/array.h"

/* ---- error trap: elog(ERROR) records its message and longjmps here ------------------------------------- */
extern jmp_buf pgshim_error_jmp;
extern int pgshim_error_armed;
const char* pgshim_last_error(void);
/* PGSHIM_TRY { ... } PGSHIM_CATCH { ... }: the body runs with the trap armed */
#define PGSHIM_TRY if ((pgshim_error_armed = 1, setjmp(pgshim_error_jmp) == 0))
#define PGSHIM_CATCH else

/* ---- arena: everything palloc'd since the last reset --------------------------------------------------- */
void pgshim_reset_memory(void);

/* ---- in-memory tables ---------------------------------------------------------------------------------- */
enum { PGSHIM_INT4 = 0, PGSHIM_FLOAT4 = 1, PGSHIM_BYTEA = 2, PGSHIM_TEXT = 3 };
typedef struct pgshim_table pgshim_table;

void pgshim_drop_tables(void);
/* a table, or (name ending in "()") a function that is selected from; columns keep the given order */
pgshim_table* pgshim_create_table(const char* name, int ncols, const char* const* colnames, const int* coltypes);
/* appends a row: bytea cells are copied from (data, bytes) pairs, text cells from C strings */
void pgshim_add_row(pgshim_table* t, const Datum* cells, const int* bytea_bytes);
/* statements seen by SPI_exec since the last pgshim_reset_memory(); a runaway loop is an ERROR */
long pgshim_statement_count(void);

bytea* pgshim_make_bytea(const void* data, int bytes);                 /* arena-allocated */
ArrayType* pgshim_make_int4_array(const int32* values, int n);         /* arena-allocated */

#endif
