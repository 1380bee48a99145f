/* executor/spi.h -- STAND-IN (see postgres.h here): the Server Programming Interface over in-memory tables. */
#ifndef PGSHIM_SPI_H
#define PGSHIM_SPI_H
#include "funcapi.h"

typedef struct SPITupleTable {
  TupleDesc tupdesc;
  HeapTuple* vals;
  uint64 numvals;
} SPITupleTable;

extern uint64 SPI_processed;
extern SPITupleTable* SPI_tuptable;

#define SPI_OK_CONNECT 1
#define SPI_OK_FINISH 2
#define SPI_OK_SELECT 5

int SPI_connect(void);
int SPI_finish(void);
int SPI_exec(const char* command, long count);
int SPI_execute(const char* command, bool read_only, long count);
Datum SPI_getbinval(HeapTuple row, TupleDesc rowdesc, int colnumber, bool* isnull);
char* SPI_getvalue(HeapTuple row, TupleDesc rowdesc, int colnumber);
void* SPI_palloc(Size size);

#endif
