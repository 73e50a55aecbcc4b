// win32_standin.cpp -- TEST INFRASTRUCTURE: the few functions behind oracle/win32_standin/windows.h.
// Linked only into oracle/_ref/ref_host.
#include "windows.h"

#include <dirent.h>

#include <string>
#include <vector>

namespace
{
std::string ForwardSlashes( const char* lpPath )
{
    std::string lPath = lpPath ? lpPath : "";
    for( char& c : lPath )
        if( c == '\\' ) c = '/';
    return lPath;
}

struct sFindState
{
    std::vector< WIN32_FIND_DATAA > maEntries;
    size_t miNext = 0;
};

std::string UpperKey( const char* lpName )
{
    std::string lKey = lpName;
    for( char& c : lKey )
        if( c >= 'a' && c <= 'z' ) c = (char)( c - 'a' + 'A' );
    return lKey;
}

bool Next( sFindState* lpState, WIN32_FIND_DATAA* lpFindData )
{
    if( !lpState || lpState->miNext >= lpState->maEntries.size() ) return false;
    *lpFindData = lpState->maEntries[ lpState->miNext++ ];
    return true;
}
} // namespace

errno_t fopen_s( FILE** lppFile, const char* lpName, const char* lpMode )
{
    *lppFile = fopen( ForwardSlashes( lpName ).c_str(), lpMode );
    return *lppFile ? 0 : errno;
}

int _mkdir( const char* lpPath ) { return mkdir( ForwardSlashes( lpPath ).c_str(), 0777 ); }

// FindFirstFileA( "<dir>/<pattern>" ).  The only patterns the reference passes are `*.*` and `*`, and on Win32 both
// match EVERY name, with or without a dot; so the pattern is not looked at.
//
// The order of enumeration is a property of the file system, not of the reference: NTFS keeps a directory as a
// B-tree keyed by the UPPER-CASED name and FindNextFile walks it in key order, so this returns the names sorted
// case-insensitively, folded to upper case, byte order within equal keys.  `.` and `..` come first, as Windows
// returns them for every directory but a drive's root.  (Folding to upper or to lower case orders names
// differently only where they hold one of  [ \ ] ^ _ `  -- the inputs recorded from this program keep those
// six characters out of the names of a directory that is enumerated.)
HANDLE FindFirstFileA( const char* lpPattern, WIN32_FIND_DATAA* lpFindData )
{
    std::string lDirectory = ForwardSlashes( lpPattern );
    const size_t liSlash = lDirectory.rfind( '/' );
    lDirectory = liSlash == std::string::npos ? std::string( "." ) : lDirectory.substr( 0, liSlash + 1 );
    DIR* lpDir = opendir( lDirectory.c_str() );
    if( !lpDir ) return INVALID_HANDLE_VALUE;

    std::vector< std::pair< std::string, WIN32_FIND_DATAA > > lNamed;
    sFindState* lpState = new sFindState;
    WIN32_FIND_DATAA lDots[ 2 ];
    bool lbDots[ 2 ] = { false, false };
    while( const dirent* lpEntry = readdir( lpDir ) )
    {
        if( strlen( lpEntry->d_name ) >= MAX_PATH ) continue; // Win32 could not have held it
        WIN32_FIND_DATAA lData;
        memset( &lData, 0, sizeof lData );
        strcpy( lData.cFileName, lpEntry->d_name );
        struct stat lInfo;
        const bool lbIsDir = stat( ( lDirectory + lpEntry->d_name ).c_str(), &lInfo ) == 0 && S_ISDIR( lInfo.st_mode );
        lData.dwFileAttributes = lbIsDir ? FILE_ATTRIBUTE_DIRECTORY : FILE_ATTRIBUTE_NORMAL;
        if( strcmp( lpEntry->d_name, "." ) == 0 ) { lDots[ 0 ] = lData; lbDots[ 0 ] = true; }
        else if( strcmp( lpEntry->d_name, ".." ) == 0 ) { lDots[ 1 ] = lData; lbDots[ 1 ] = true; }
        else lNamed.emplace_back( UpperKey( lpEntry->d_name ), lData );
    }
    closedir( lpDir );
    std::sort( lNamed.begin(), lNamed.end(), []( const auto& a, const auto& b ) {
        return a.first != b.first ? a.first < b.first : strcmp( a.second.cFileName, b.second.cFileName ) < 0;
    } );
    for( int ii = 0; ii < 2; ++ii )
        if( lbDots[ ii ] ) lpState->maEntries.push_back( lDots[ ii ] );
    for( const auto& lEntry : lNamed ) lpState->maEntries.push_back( lEntry.second );

    if( !Next( lpState, lpFindData ) )
    {
        delete lpState;
        return INVALID_HANDLE_VALUE;
    }
    return lpState;
}

int FindNextFileA( HANDLE lHandle, WIN32_FIND_DATAA* lpFindData )
{
    if( lHandle == INVALID_HANDLE_VALUE ) return 0;
    return Next( static_cast< sFindState* >( lHandle ), lpFindData ) ? 1 : 0;
}

int FindClose( HANDLE lHandle )
{
    if( lHandle == INVALID_HANDLE_VALUE ) return 0;
    delete static_cast< sFindState* >( lHandle );
    return 1;
}
