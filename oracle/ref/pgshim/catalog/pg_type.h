/* catalog/pg_type.h -- STAND-IN (see postgres.h here): the type OIDs the reference names. */
#ifndef PGSHIM_PG_TYPE_H
#define PGSHIM_PG_TYPE_H
#define BOOLOID 16
#define BYTEAOID 17
#define INT2OID 21
#define INT4OID 23
#define TEXTOID 25
#define FLOAT4OID 700
#define FLOAT8OID 701
#endif
