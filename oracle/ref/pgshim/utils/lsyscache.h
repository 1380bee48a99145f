/* utils/lsyscache.h -- STAND-IN (see postgres.h here). */
#ifndef PGSHIM_LSYSCACHE_H
#define PGSHIM_LSYSCACHE_H
#include "postgres.h"
void get_typlenbyvalalign(Oid typid, int16* typlen, bool* typbyval, char* typalign);
#endif
