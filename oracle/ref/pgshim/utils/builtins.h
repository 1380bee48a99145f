/* utils/builtins.h -- STAND-IN (see postgres.h here): the reference includes it and uses nothing from it
 * beyond what utils/lsyscache.h declares. */
#ifndef PGSHIM_BUILTINS_H
#define PGSHIM_BUILTINS_H
#include "postgres.h"
#include "utils/lsyscache.h"
#endif
